// Pins the rule of the per-row selection (legion_amd/csrc/topk_rule.h: the exponential variate, the float ordering, the three keys,
// eligibility, which calls legion_row_topk and legion_topk_keys refuse, and the scratch size) over a literal table.  The variates and
// keys were computed with tests/topk_ref.py (numpy, np.frexp, one operation at a time), the codes written down from the rules as
// include/legion_hip.h documents them; none comes from the header.
//   g++ -O1 -std=c++17 topk_rule_test.cpp -o t && ./t
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../legion_amd/csrc/topk_rule.h"

static_assert(LEGION_IN_EDGES_MAX_ROWS == 1048576 && LEGION_TOPK_MAX_K == 64, "the tables below spell the limits out");
static_assert(topk_exp_variate(0) > 36.7 && topk_exp_variate(0) < 36.8 && topk_float_order(0.0f) == 0x80000000u,
              "the rule is constexpr: the device runs this text");
static_assert(LG_TOPK_LONG == 4096 && LG_TOPK_GRID == 2048 && LG_TOPK_LONG_GRID == 256, "tests/topk_ref.py spells the kernels' constants out");
enum { OK, CNT, MANY, KSM, KLG, MODE, WGT, PTR, SCR };
static const int64_t BIG = (int64_t)1 << 40;
static const float INF = std::numeric_limits<float>::infinity();
static const float QNAN = std::numeric_limits<float>::quiet_NaN();
static const float DEN = 1.401298464324817e-45f;                   // the smallest denormal
static const float FMAX = 3.4028234663852886e38f;

static uint64_t bits(double d) { return __builtin_bit_cast(uint64_t, d); }

struct VariateCase { uint64_t x; uint64_t want; };
static const VariateCase variates[] = {
    {0x0000000000000000ull, 0x40425e4f7b2737faull},                // 36.7368005696771 = 53 ln 2: u = 2^-53 folds to m = 1
    {0xffffffffffffffffull, 0x3ca0000000000000ull},                // 1.1102230246251565e-16 = 2^-53
    {0x0000000000001000ull, 0x4041d1b02751cfe1ull},                // j = 1
    {0x8000000000000000ull, 0x3fe62e42fefa39edull},                // just above u = 1/2
    {0x7fffffffffffffffull, 0x3fe62e42fefa39f1ull},                // just below
    {0xb504f333f9de5000ull, 0x3fd62e42fefa39f4ull},                // the last m below SQ: folded
    {0xb504f333f9de6000ull, 0x3fd62e42fefa39eeull},                // the first m not below it
    {0xb504f333f9df0000ull, 0x3fd62e42fefa39b6ull},                // where the z^10 term decides the last bit
    {0xb504f333f9dfc000ull, 0x3fd62e42fefa3972ull},
    {0x123456789abcdef0ull, 0x400525e973a05652ull},
};

struct ExpCase { int64_t e; int64_t salt; uint64_t want; };
static const ExpCase exps[] = {
    {0LL, 0LL, 0x3fdb5458a89b6fadull}, {1000LL, 3LL, 0x3fe26060f6f5d67aull}, {5LL, -1LL, 0x3ff9153ae4767625ull},
    {4294967303LL, 12345LL, 0x3ffcf93730223571ull}, {1099511627776LL, -9223372036854775807LL - 1, 0x3fd30f43e4c222beull},
    {123456789LL, 9223372036854775807LL, 0x3ff1fcfe635138e2ull},
};

struct OrderCase { float w; uint32_t want; };
static const OrderCase orders[] = {
    {0.0f, 0x80000000u}, {-0.0f, 0x80000000u}, {DEN, 0x80000001u}, {-DEN, 0x7ffffffeu}, {INF, 0xff800000u}, {-INF, 0x007fffffu},
    {FMAX, 0xff7fffffu}, {-FMAX, 0x00800000u}, {1.0f, 0xbf800000u}, {-1.0f, 0x407fffffu}, {0.125f, 0xbe000000u}, {2.5f, 0xc0200000u},
    {1.1754942e-38f, 0x807fffffu},
};

struct KeyCase { int32_t mode; int64_t e; float w; int64_t salt; uint64_t want; };
static const KeyCase keycases[] = {
    {0, 7LL, 2.5f, 0LL, 0x000000003fdfffffull}, {1, 7LL, 2.5f, 0LL, 0x00000000c0200000ull}, {0, 7LL, -0.0f, 0LL, 0x000000007fffffffull},
    {1, 7LL, -0.0f, 0LL, 0x0000000080000000ull}, {0, 7LL, 0.0f, 0LL, 0x000000007fffffffull}, {0, 7LL, INF, 0LL, 0x00000000007fffffull},
    {1, 7LL, -INF, 0LL, 0x00000000007fffffull},
    {2, 1000LL, 0.125f, 3LL, 0x40126060f6f5d67aull}, {2, 1001LL, 1.0f, 3LL, 0x3fde086fc69fa454ull}, {2, 5LL, DEN, -1LL, 0x4949153ae4767625ull},
    {2, 4294967303LL, FMAX, 12345LL, 0x37fcf9374d1b6cbeull}, {2, 1004LL, 4.0f, 199999LL, 0x3fea7fae7313df1bull},
};

struct EligibleCase { int32_t mode; int32_t src; float w; bool has_w; bool want; };
static const EligibleCase eligibles[] = {
    {0, 5, 1.0f, true, true}, {0, -1, 1.0f, true, false}, {0, 0, QNAN, true, false}, {0, 0, -QNAN, true, false}, {0, 0, INF, true, true},
    {0, 0, -INF, true, true}, {0, 0, -1.0f, true, true}, {0, 0, 0.0f, true, true}, {1, 2147483647, -0.0f, true, true}, {1, 3, QNAN, true, false},
    {1, -1, 0.0f, true, false}, {1, -2147483647 - 1, 0.0f, true, false},
    {2, 5, 1.0f, true, true}, {2, 5, DEN, true, true}, {2, 5, FMAX, true, true}, {2, 5, 0.0f, true, false}, {2, 5, -0.0f, true, false},
    {2, 5, -1.0f, true, false}, {2, 5, INF, true, false}, {2, 5, -INF, true, false}, {2, 5, QNAN, true, false}, {2, -1, 1.0f, true, false},
    {2, 5, QNAN, false, true}, {2, 0, 0.0f, false, true}, {2, -1, 1.0f, false, false},
};

struct RowCase { int32_t n; int32_t k; int32_t mode; bool has_w; bool ptrs; int64_t scratch; int want; };
static const RowCase rowcases[] = {
    // n, k, mode, w given, pointers given, scratch_bytes -> code
    {100, 10, 0, true, true, 404, OK}, {100, 10, 0, true, true, 403, SCR}, {100, 10, 0, true, true, 0, SCR}, {100, 10, 0, true, true, -1, SCR},
    {0, 1, 2, false, true, 4, OK}, {0, 1, 2, false, true, 3, SCR}, {1048576, 64, 1, true, true, 4194308, OK}, {1048576, 64, 1, true, true, 4194307, SCR},
    {-1, 10, 0, true, true, BIG, CNT}, {-2147483647 - 1, 10, 0, true, true, BIG, CNT}, {1048577, 10, 0, true, true, BIG, MANY},
    {2147483647, 10, 0, true, true, BIG, MANY},
    {100, 0, 0, true, true, BIG, KSM}, {100, -1, 0, true, true, BIG, KSM}, {100, 1, 0, true, true, BIG, OK},
    {100, 64, 0, true, true, BIG, OK}, {100, 65, 0, true, true, BIG, KLG}, {100, 2147483647, 0, true, true, BIG, KLG},
    {100, 10, -1, true, true, BIG, MODE}, {100, 10, 3, true, true, BIG, MODE}, {100, 10, 2, true, true, BIG, OK}, {100, 10, 1, true, true, BIG, OK},
    {100, 10, 0, false, true, BIG, WGT}, {100, 10, 1, false, true, BIG, WGT}, {100, 10, 2, false, true, BIG, OK},
    {100, 10, 2, false, false, BIG, PTR}, {100, 10, 0, true, false, BIG, PTR},
    // the order of the checks: n, n, k, k, mode, w, pointers, scratch
    {-1, 0, 3, false, false, -1, CNT}, {1048577, 0, 3, false, false, -1, MANY}, {100, 0, 3, false, false, -1, KSM}, {100, 65, 3, false, false, -1, KLG},
    {100, 64, 3, false, false, -1, MODE}, {100, 64, 0, false, false, -1, WGT}, {100, 64, 2, false, false, -1, PTR}, {100, 64, 2, false, true, -1, SCR},
};

struct KeysCase { int64_t n; int32_t mode; bool has_w; bool ptrs; int want; };
static const KeysCase keyscases[] = {
    {100, 0, true, true, OK}, {0, 2, false, true, OK}, {2147483647LL, 1, true, true, OK}, {2147483648LL, 1, true, true, MANY}, {-1, 0, true, true, CNT},
    {100, 3, true, true, MODE}, {100, -1, true, true, MODE}, {100, 0, false, true, WGT}, {100, 2, false, false, PTR},
    {-1, 3, false, false, CNT}, {BIG, 3, false, false, MANY}, {100, 3, false, false, MODE}, {100, 1, false, false, WGT},
};

struct BytesCase { int32_t n; int64_t want; };
static const BytesCase sizes[] = {
    {0, 4}, {1, 8}, {1048576, 4194308}, {1048577, -1}, {-1, -1}, {2147483647, -1},
};

static int code(TopkRefusal r)
{
    switch (r) {
    case TopkRefusal::Ok: return OK;
    case TopkRefusal::Count: return CNT;
    case TopkRefusal::TooMany: return MANY;
    case TopkRefusal::KSmall: return KSM;
    case TopkRefusal::KLarge: return KLG;
    case TopkRefusal::Mode: return MODE;
    case TopkRefusal::Weights: return WGT;
    case TopkRefusal::Pointer: return PTR;
    case TopkRefusal::Scratch: return SCR;
    }
    return -1;
}

int main()
{
    int bad = 0, n = 0;
    for (const VariateCase& c : variates) {
        n++;
        const double E = topk_exp_variate(c.x);
        const double u = (double)(2 * (c.x >> 12) + 1) * 0x1p-53;
        if (bits(E) != c.want) {
            printf("MISMATCH topk_exp_variate(%016llx): got %016llx, want %016llx\n", (unsigned long long)c.x, (unsigned long long)bits(E),
                   (unsigned long long)c.want);
            bad++;
        }
        if (!(E > 0.0 && E < 37.0) || std::fabs(E + std::log(u)) > 1e-15 * std::fabs(std::log(u))) {
            printf("MISMATCH: the table itself at %016llx: %.17g is not -ln %.17g\n", (unsigned long long)c.x, E, u);
            bad++;
        }
    }
    for (const ExpCase& c : exps) {
        n++;
        if (bits(topk_exp(c.e, c.salt)) != c.want || bits(topk_exp_keyed(labor_key(c.salt), c.e)) != c.want) {
            printf("MISMATCH topk_exp(%lld, %lld): got %016llx, want %016llx\n", (long long)c.e, (long long)c.salt,
                   (unsigned long long)bits(topk_exp(c.e, c.salt)), (unsigned long long)c.want);
            bad++;
        }
    }
    for (const OrderCase& c : orders) {
        n++;
        if (topk_float_order(c.w) != c.want) {
            printf("MISMATCH topk_float_order(%g): got %08x, want %08x\n", c.w, topk_float_order(c.w), c.want);
            bad++;
        }
    }
    // the order is the floats': every pair of the table
    for (const OrderCase& a : orders)
        for (const OrderCase& b : orders)
            if ((a.w < b.w) != (topk_float_order(a.w) < topk_float_order(b.w))) {
                printf("MISMATCH: the order of %g and %g\n", a.w, b.w);
                bad++;
            }
    for (const KeyCase& c : keycases) {
        n++;
        const uint64_t got = topk_key(c.mode, c.w, labor_key(c.salt), c.e);
        if (got != c.want || got == TOPK_NO_KEY) {
            printf("MISMATCH topk_key(mode %d, e %lld, w %g, salt %lld): got %016llx, want %016llx\n", c.mode, (long long)c.e, c.w,
                   (long long)c.salt, (unsigned long long)got, (unsigned long long)c.want);
            bad++;
        }
    }
    for (const EligibleCase& c : eligibles) {
        n++;
        if (topk_eligible(c.mode, c.src, c.w, c.has_w) != c.want) {
            printf("MISMATCH topk_eligible(mode %d, src %d, w %g, has_w %d): want %d\n", c.mode, c.src, c.w, c.has_w, c.want);
            bad++;
        }
    }
    for (const RowCase& c : rowcases) {
        n++;
        const TopkRefusal r = topk_refusal(c.n, c.k, c.mode, c.has_w, c.ptrs, c.scratch);
        if (code(r) != c.want) {
            printf("MISMATCH row_topk n %d k %d mode %d w %d pointers %d scratch %lld: got %d, want %d\n", c.n, c.k, c.mode, c.has_w, c.ptrs,
                   (long long)c.scratch, code(r), c.want);
            bad++;
        }
        if (topk_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const KeysCase& c : keyscases) {
        n++;
        const TopkRefusal r = topk_keys_refusal(c.n, c.mode, c.has_w, c.ptrs);
        if (code(r) != c.want) {
            printf("MISMATCH topk_keys n %lld mode %d w %d pointers %d: got %d, want %d\n", (long long)c.n, c.mode, c.has_w, c.ptrs, code(r), c.want);
            bad++;
        }
    }
    for (const BytesCase& c : sizes) {
        n++;
        if (topk_scratch_bytes(c.n) != c.want) {
            printf("MISMATCH scratch bytes of %d: got %lld, want %lld\n", c.n, (long long)topk_scratch_bytes(c.n), (long long)c.want);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
