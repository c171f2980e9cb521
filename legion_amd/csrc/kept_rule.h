// kept_rule.h -- the scratch of a kept-slot compaction (legion_labor_count / legion_labor_edges, legion_induced_count /
// legion_induced_edges, include/legion_hip.h; the kernels: kept_slots.h): how many tiles and second-level sums m slots make and how
// many bytes they take.  No HIP, all constexpr: labor_rule.h and induced_rule.h put their own limit on m in front of it,
// tests/cpu/labor_rule_test.cpp and tests/cpu/induced_rule_test.cpp pin it over literal tables with g++.  (A classic guard: a table that
// includes a changed copy of this file first shadows this one where the rule headers include it.)
#ifndef LEGION_KEPT_RULE_H
#define LEGION_KEPT_RULE_H

#include <cstdint>

// the tiles of 1 024 slots whose kept counts are summed: at most 2^20 (m in [0, 2^30])
constexpr int64_t kept_tiles(int64_t m) { return (m + 1023) / 1024; }
// the sums of 256 tile counts the one-workgroup scan takes: at most 4 096
constexpr int64_t kept_groups(int64_t m) { return (kept_tiles(m) + 255) / 256; }

// one int64 per tile plus one (the total), plus one int64 per 256 tiles
constexpr int64_t kept_scratch_bytes(int64_t m) { return 8 * (kept_tiles(m) + 1 + kept_groups(m)); }

static_assert(kept_groups((int64_t)1 << 30) == 4096, "2^20 tile counts make 4 096 second-level sums, the one-workgroup scan's reach");

#endif
