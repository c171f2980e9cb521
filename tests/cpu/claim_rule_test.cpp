// Pins the bit formats of a sampled hop (legion_amd/csrc/claim_rule.h: the hash with its bucket and sub-bucket bits, the claim pair, the
// place of a claim in the interleaved lists, the de-duplication's table words and what a surviving word says, the losers' codes in
// slot_pos and slot_dst, the compaction's look-back word) over literal tables and the properties the kernels rest on.  The hash and home
// values were computed with numpy (tests/test_claim_rule_cpu.py computes them again); none comes from the header.
//   g++ -O1 -std=c++17 claim_rule_test.cpp -o t && ./t
#include <cstdio>
#include <vector>

#include "../../legion_amd/csrc/claim_rule.h"

static_assert(lg_tab_hash(0) == 0u && lg_claim_at(0, 0, 8) == 0 && st_status(LG_ST_PREF) == 2u && !lg_tab_first_touch(0u, 0u),
              "the rule is constexpr: the device runs this text");
static_assert(LG_CLAIM_CHUNK == 512, "the tables below spell the chunk out");
static const int32_t I32_MAX = 2147483647, I32_MIN = -2147483647 - 1, V_MAX = 2147483646;      // V_MAX: the largest vertex and slot the codes hold

struct HashCase { int32_t v; uint32_t want; };
static const HashCase hashes[] = {
    {0, 0x00000000u}, {1, 0x688990c0u}, {-1, 0x6768824au}, {2147483647, 0x8d29ffb8u}, {-2147483647 - 1, 0xcc4b4124u},
    {123456, 0xbd2111c0u}, {1000000007, 0x4d6507adu},
};

struct HomeCase { uint32_t h; int32_t tb; uint32_t want; };
static const HomeCase homes[] = {
    {0x00000001u, 13, 5062}, {0xdeadbeefu, 13, 5015}, {0x00000001u, 14, 10125}, {0xdeadbeefu, 14, 10030},
};

static int bad = 0, n = 0;
#define CHECK(cond, ...)                                                                                                                   \
    do {                                                                                                                                   \
        n++;                                                                                                                               \
        if (!(cond)) { printf("MISMATCH %s: ", #cond); printf(__VA_ARGS__); printf("\n"); bad++; }                                         \
    } while (0)

int main()
{
    // the hash
    for (const HashCase& c : hashes) CHECK(lg_tab_hash(c.v) == c.want, "lg_tab_hash(%d) = %08x, want %08x", c.v, lg_tab_hash(c.v), c.want);

    // the pair
    const int32_t vs[] = {0, 1, V_MAX};
    const uint32_t vals[] = {0u, 0x7fffffffu};
    for (int32_t v : vs)
        for (uint32_t x : vals) {
            const uint64_t w = lg_pair(v, x);
            CHECK(lg_pair_vertex(w) == v && lg_pair_value(w) == x, "pair(%d, %u) reads back (%d, %u)", v, x, lg_pair_vertex(w), lg_pair_value(w));
            CHECK(w != LG_PAIR_EMPTY, "pair(%d, %u) is the empty word", v, x);
        }
    CHECK(lg_pair(I32_MAX, 0xffffffffu) != LG_PAIR_EMPTY && LG_PAIR_EMPTY == 0xffffffffffffffffull, "no vertex >= 0 makes the empty word");
    CHECK(lg_pair(5, 7u) == 0x0000000500000007ull, "pair(5, 7) = %016llx", (unsigned long long)lg_pair(5, 7u));

    // the table words: per vertex the lowest survives -- known below every claim, claims by slot, empty above all, vertices by vertex
    CHECK(lg_tab_known(5, 7u) == 0x0000000500000007ull && lg_tab_claim(5, 7u) == 0x0000000580000007ull, "known / claim (5, 7) = %016llx / %016llx",
          (unsigned long long)lg_tab_known(5, 7u), (unsigned long long)lg_tab_claim(5, 7u));
    for (int32_t v : vs) {
        CHECK(lg_tab_known(v, 0x7fffffffu) < lg_tab_claim(v, 0u), "vertex %d: the highest known position is not below the lowest claim", v);
        CHECK(lg_tab_known(v, 0u) < lg_tab_known(v, 1u), "vertex %d: known words do not order by position", v);
        CHECK(lg_tab_claim(v, 0u) < lg_tab_claim(v, 1u) && lg_tab_claim(v, 1u) < lg_tab_claim(v, (uint32_t)V_MAX), "vertex %d: claims do not order by slot", v);
        CHECK(lg_tab_claim(v, (uint32_t)V_MAX) < LG_PAIR_EMPTY, "vertex %d: the empty word is not above its highest claim", v);
        CHECK(lg_pair_vertex(lg_tab_claim(v, 9u)) == v && lg_pair_vertex(lg_tab_known(v, 9u)) == v, "vertex %d: a word does not keep its vertex", v);
    }
    CHECK(lg_tab_claim(0, (uint32_t)V_MAX) < lg_tab_known(1, 0u) && lg_tab_claim(1, (uint32_t)V_MAX) < lg_tab_known(V_MAX, 0u), "words of different vertices do not order by vertex");

    // what a surviving word says about the claim of a slot
    for (uint32_t slot : {0u, 7u, (uint32_t)V_MAX}) {
        const uint32_t mine = lg_pair_value(lg_tab_claim(3, slot));
        CHECK(lg_tab_first_touch(mine, slot), "slot %u: its own surviving word is not a first touch", slot);
        for (uint32_t pos : {0u, 0x7fffffffu}) {
            const uint32_t known = lg_pair_value(lg_tab_known(3, pos));
            CHECK(!lg_tab_first_touch(known, slot) && lg_tab_loser_pos(known) == (int32_t)pos, "slot %u lost to the known position %u: %d", slot, pos, lg_tab_loser_pos(known));
        }
        if (slot > 0) {
            for (uint32_t s : {0u, slot - 1u}) {
                const uint32_t other = lg_pair_value(lg_tab_claim(3, s));
                CHECK(!lg_tab_first_touch(other, slot), "slot %u: the surviving word of slot %u reads as its first touch", slot, s);
                CHECK(lg_tab_loser_pos(other) == lg_pos_lost_to((int32_t)s) && lg_tab_loser_pos(other) < LG_POS_NONE && lg_pos_winner(lg_tab_loser_pos(other)) == (int32_t)s,
                      "slot %u lost to slot %u: code %d", slot, s, lg_tab_loser_pos(other));
            }
        }
    }

    // the home of a hash
    for (const HomeCase& c : homes) CHECK(lg_tab_home(c.h, c.tb) == c.want, "home(%08x, %d) = %u, want %u", c.h, c.tb, lg_tab_home(c.h, c.tb), c.want);
    for (int32_t tb : {13, 14})
        for (uint32_t h : {0u, 1u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0x12345678u})
            CHECK(lg_tab_home(h, tb) < (1u << tb), "home(%08x, %d) = %u lies outside the table", h, tb, lg_tab_home(h, tb));

    // bucket and sub-bucket: disjoint bits of the hash, the bucket's the lowest
    for (int32_t bb : {3, 4, 6, 8})
        for (uint32_t passes : {1u, 2u, 1u << 14})
            for (uint32_t h : {0u, 0xffffffffu, 0x12345678u, 0xdeadbeefu, (1u << bb) - 1u, 1u << bb}) {
                const int32_t nb = 1 << bb;
                const uint32_t b = (uint32_t)lg_hash_bucket(h, nb), s = lg_sub_bucket(h, bb, passes);
                CHECK(b < (uint32_t)nb && s < passes, "bb %d passes %u h %08x: bucket %u sub-bucket %u out of range", bb, passes, h, b, s);
                CHECK((b | (s << bb)) == (h & ((uint32_t)nb * passes - 1u)), "bb %d passes %u h %08x: bucket %u and sub-bucket %u are not the hash's low bits", bb, passes, h, b, s);
            }
    CHECK(lg_bucket(1, 8) == 0 && lg_bucket(1, 256) == 0xc0 && lg_bucket(-1, 64) == 0x0a, "the bucket of a vertex is its hash's: %d %d %d", lg_bucket(1, 8), lg_bucket(1, 256), lg_bucket(-1, 64));
    CHECK(lg_sub_bucket(0x688990c0u, 8, 1u << 14) == 0x0990u && lg_sub_bucket(0x688990c0u, 3, 2u) == 0u && lg_sub_bucket(0x688990c8u, 3, 2u) == 1u, "sub-bucket literals");

    // the claim lists: every (b, k) its own place below what the pool plan allocates, neighbours inside a chunk adjacent
    CHECK(lg_claim_at(1, 512, 8) == 4608 && lg_claim_at(0, 0, 8) == 0 && lg_claim_at(7, 511, 8) == 4095 && lg_claim_at(255, 1535, 256) == 393215, "claim-list literals: %lld",
          (long long)lg_claim_at(1, 512, 8));
    for (int32_t nb : {8, 16, 64, 256})
        for (int32_t chunks : {1, 3}) {
            const int64_t size = (int64_t)nb * chunks * LG_CLAIM_CHUNK;
            std::vector<char> seen((size_t)size, 0);
            int64_t wrong = 0;
            for (int32_t b = 0; b < nb; b++)
                for (int32_t k = 0; k < chunks * LG_CLAIM_CHUNK; k++) {
                    const int64_t at = lg_claim_at(b, k, nb);
                    if (at < 0 || at >= size || seen[(size_t)at]) { wrong++; continue; }
                    seen[(size_t)at] = 1;
                    if ((k & (LG_CLAIM_CHUNK - 1)) != LG_CLAIM_CHUNK - 1 && lg_claim_at(b, k + 1, nb) != at + 1) wrong++;
                }
            CHECK(wrong == 0, "%d lists of %d chunks: %lld places out of range, taken twice or not adjacent", nb, chunks, (long long)wrong);
        }

    // the loser's mark in slot_dst and its code in slot_pos
    for (int32_t v : {0, 1, 12345, V_MAX}) {
        CHECK(LG_SLOT_LOSER(LG_SLOT_LOSER(v)) == v && LG_SLOT_LOSER(v) <= -2 && LG_SLOT_LOSER(v) >= I32_MIN, "LG_SLOT_LOSER(%d) = %d", v, LG_SLOT_LOSER(v));
        CHECK(lg_pos_winner(lg_pos_lost_to(v)) == v && lg_pos_lost_to(v) < LG_POS_NONE, "lost to slot %d: code %d", v, lg_pos_lost_to(v));
    }
    CHECK(LG_SLOT_LOSER(0) == -2 && LG_SLOT_LOSER(V_MAX) == I32_MIN && lg_pos_lost_to(0) == -2 && lg_pos_lost_to(V_MAX) == I32_MIN && LG_POS_NONE == -1, "the ends of the codes");

    // the look-back word
    for (uint64_t status : {(uint64_t)LG_ST_AGG, (uint64_t)LG_ST_PREF})
        for (int32_t e : {0, I32_MAX})
            for (int32_t m : {0, I32_MAX}) {
                const uint64_t w = st_word(status, e, m);
                CHECK(st_edges(w) == e && st_nodes(w) == m && st_status(w) == (uint32_t)(status >> 62) && st_status(w) != 0u, "st_word(%u, %d, %d) reads back (%u, %d, %d)",
                      (uint32_t)(status >> 62), e, m, st_status(w), st_edges(w), st_nodes(w));
            }
    CHECK(st_status(0ull) == 0u && st_status(LG_ST_AGG) == 1u && st_status(LG_ST_PREF) == 2u, "the zero word reads as not written");
    CHECK(st_word(LG_ST_PREF, 3, 5) == 0x8000000180000005ull, "st_word(PREF, 3, 5) = %016llx", (unsigned long long)st_word(LG_ST_PREF, 3, 5));

    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
