// Pins the argument rule of node2vec walks (legion_amd/csrc/node2vec_rule.h: node2vec_refusal, which calls legion_node2vec_walk refuses;
// node2vec_bias, what p and q become for the kernel) over a literal table.  The expected codes were written down from the rule as
// include/legion_hip.h documents it, not from the header.
//   g++ -O1 -std=c++17 node2vec_rule_test.cpp -o t && ./t
#include <cmath>
#include <cstdio>
#include <limits>

#include "../../legion_amd/csrc/node2vec_rule.h"

static_assert(LEGION_NODE2VEC_MAX_TRIES == 256 && LEGION_NODE2VEC_MAX_BIAS == 16, "the table below spells both limits out");
enum { OK, CNT, IDX, WGT, TAB, TRY, BIAS, RATIO, SORT };

static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();
static const int64_t M31 = 2147483647;

struct Case { int32_t n, length; int64_t base; int32_t weighted, table, tries; float p, q; int32_t sorted; int want; };
static const Case cases[] = {
    // walks, length, base, weighted, graph has a table, max_tries, p, q, rows checked sorted -> code
    {8, 4, 0, 0, 0, 256, 1.0f, 1.0f, 1, OK}, {8, 4, 0, 1, 1, 256, 1.0f, 1.0f, 1, OK}, {0, 4, 0, 0, 0, 1, 0.5f, 2.0f, 1, OK},
    {8, 4, 0, 0, 1, 1, 4.0f, 0.25f, 1, OK}, {8, 4, 0, 0, 0, 2, 0.25f, 4.0f, 1, OK}, {8, 4, 0, 0, 0, 255, 16.0f, 1.0f, 1, OK},
    // counts and the draw index
    {-1, 4, 0, 0, 0, 256, 1.0f, 1.0f, 1, CNT}, {8, 0, 0, 0, 0, 256, 1.0f, 1.0f, 1, CNT}, {8, -2, 0, 0, 0, 256, 1.0f, 1.0f, 1, CNT},
    {8, 4, -1, 0, 0, 256, 1.0f, 1.0f, 1, CNT},
    {8, 4, M31 - 32, 0, 0, 256, 1.0f, 1.0f, 1, OK}, {8, 4, M31 - 31, 0, 0, 256, 1.0f, 1.0f, 1, IDX}, {0, 4, M31, 0, 0, 256, 1.0f, 1.0f, 1, OK},
    {2147483647, 2, 0, 0, 0, 256, 1.0f, 1.0f, 1, IDX}, {2147483647, 1, 0, 0, 0, 256, 1.0f, 1.0f, 1, OK}, {2147483647, 1, 1, 0, 0, 256, 1.0f, 1.0f, 1, IDX},
    {2147483647, 2147483647, 0, 0, 0, 256, 1.0f, 1.0f, 1, IDX},
    // weighted
    {8, 4, 0, 2, 1, 256, 1.0f, 1.0f, 1, WGT}, {8, 4, 0, -1, 1, 256, 1.0f, 1.0f, 1, WGT}, {8, 4, 0, 1, 0, 256, 1.0f, 1.0f, 1, TAB},
    // tries
    {8, 4, 0, 0, 0, 0, 1.0f, 1.0f, 1, TRY}, {8, 4, 0, 0, 0, -1, 1.0f, 1.0f, 1, TRY}, {8, 4, 0, 0, 0, 257, 1.0f, 1.0f, 1, TRY},
    {8, 4, 0, 0, 0, 1, 1.0f, 1.0f, 1, OK},
    // p, q: finite and > 0
    {8, 4, 0, 0, 0, 256, 0.0f, 1.0f, 1, BIAS}, {8, 4, 0, 0, 0, 256, 1.0f, 0.0f, 1, BIAS}, {8, 4, 0, 0, 0, 256, -1.0f, 1.0f, 1, BIAS},
    {8, 4, 0, 0, 0, 256, 1.0f, -0.5f, 1, BIAS}, {8, 4, 0, 0, 0, 256, NaN, 1.0f, 1, BIAS}, {8, 4, 0, 0, 0, 256, 1.0f, NaN, 1, BIAS},
    {8, 4, 0, 0, 0, 256, Inf, 1.0f, 1, BIAS}, {8, 4, 0, 0, 0, 256, 1.0f, Inf, 1, BIAS}, {8, 4, 0, 0, 0, 256, -Inf, 1.0f, 1, BIAS},
    // the ratio of the largest to the smallest of 1/p, 1, 1/q: at most 16
    {8, 4, 0, 0, 0, 256, 16.0f, 1.0f, 1, OK}, {8, 4, 0, 0, 0, 256, 1.0f, 16.0f, 1, OK}, {8, 4, 0, 0, 0, 256, 0.0625f, 1.0f, 1, OK},
    {8, 4, 0, 0, 0, 256, 1.0f, 0.0625f, 1, OK}, {8, 4, 0, 0, 0, 256, 4.0f, 0.25f, 1, OK}, {8, 4, 0, 0, 0, 256, 0.25f, 4.0f, 1, OK},
    {8, 4, 0, 0, 0, 256, 16.5f, 1.0f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 1.0f, 17.0f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 0.0624f, 1.0f, 1, RATIO},
    {8, 4, 0, 0, 0, 256, 1.0f, 0.05f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 8.0f, 0.25f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 0.25f, 8.0f, 1, RATIO},
    {8, 4, 0, 0, 0, 256, 1e-30f, 1e-30f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 1e30f, 1e30f, 1, RATIO}, {8, 4, 0, 0, 0, 256, 100.0f, 100.0f, 1, RATIO},
    {8, 4, 0, 0, 0, 256, 0.01f, 0.01f, 1, RATIO},
    // the graph's rows: checked and sorted, nothing less
    {8, 4, 0, 0, 0, 256, 1.0f, 1.0f, 0, SORT}, {8, 4, 0, 0, 0, 256, 1.0f, 1.0f, -1, SORT}, {0, 4, 0, 0, 0, 256, 1.0f, 1.0f, -1, SORT},
    // the order of the checks: the first rule that fails names the refusal
    {-1, 4, 0, 2, 0, 0, NaN, 1.0f, 0, CNT}, {8, 4, M31, 2, 0, 0, NaN, 1.0f, 0, IDX}, {8, 4, 0, 2, 0, 0, NaN, 1.0f, 0, WGT},
    {8, 4, 0, 1, 0, 0, NaN, 1.0f, 0, TAB}, {8, 4, 0, 0, 0, 0, NaN, 1.0f, 0, TRY}, {8, 4, 0, 0, 0, 1, NaN, 1.0f, 0, BIAS},
    {8, 4, 0, 0, 0, 1, 32.0f, 1.0f, 0, RATIO},
};

static int code(Node2vecRefusal r)
{
    switch (r) {
    case Node2vecRefusal::Ok: return OK;
    case Node2vecRefusal::Count: return CNT;
    case Node2vecRefusal::DrawIndex: return IDX;
    case Node2vecRefusal::Weighted: return WGT;
    case Node2vecRefusal::NoTable: return TAB;
    case Node2vecRefusal::Tries: return TRY;
    case Node2vecRefusal::Bias: return BIAS;
    case Node2vecRefusal::BiasRatio: return RATIO;
    case Node2vecRefusal::Unsorted: return SORT;
    }
    return -1;
}

struct BiasCase { float p, q; double a, b, mx, lo, hi; };
static const BiasCase biases[] = {
    {1.0f, 1.0f, 1.0, 1.0, 1.0, 1.0, 1.0}, {0.5f, 2.0f, 2.0, 0.5, 2.0, 0.5, 1.0}, {4.0f, 0.25f, 0.25, 4.0, 4.0, 1.0, 4.0},
    {0.25f, 4.0f, 4.0, 0.25, 4.0, 0.25, 1.0}, {16.0f, 1.0f, 0.0625, 1.0, 1.0, 1.0, 1.0}, {2.0f, 0.5f, 0.5, 2.0, 2.0, 1.0, 2.0},
    {3.0f, 1.0f, 1.0 / 3.0, 1.0, 1.0, 1.0, 1.0}, {0.1f, 1.0f, 1.0 / (double)0.1f, 1.0, 1.0 / (double)0.1f, 1.0, 1.0},
};

int main()
{
    int bad = 0, n = 0;
    for (const Case& c : cases) {
        n++;
        const Node2vecRefusal r = node2vec_refusal(c.n, c.length, c.base, c.weighted, c.table != 0, c.tries, c.p, c.q, c.sorted);
        if (code(r) != c.want) {
            printf("MISMATCH walks %d length %d base %lld weighted %d table %d tries %d p %g q %g sorted %d: got %d, want %d\n", c.n, c.length,
                   (long long)c.base, c.weighted, c.table, c.tries, (double)c.p, (double)c.q, c.sorted, code(r), c.want);
            bad++;
        }
        if (node2vec_refusal_text(r)[0] == 0) { printf("MISMATCH: a reason without a text\n"); bad++; }
    }
    for (const BiasCase& c : biases) {
        n++;
        const Node2vecBias w = node2vec_bias(c.p, c.q);
        if (w.a != c.a || w.b != c.b || w.mx != c.mx || w.lo != c.lo || w.hi != c.hi) {
            printf("MISMATCH bias p %g q %g: got a %.17g b %.17g mx %.17g lo %.17g hi %.17g\n", (double)c.p, (double)c.q, w.a, w.b, w.mx, w.lo, w.hi);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
