// Pins the host rule of the sparse row update's sort (legion_amd/csrc/update_rule.h: the bit width of N and the passes of 8 bits)
// over a literal table, written down from the rule as include/legion_hip.h and DESIGN.md 4.30 state it.
//   g++ -O1 -std=c++17 -I include update_rule_test.cpp -o t && ./t
#include <cstdio>

#include "../../legion_amd/csrc/update_rule.h"

struct WidthCase { int32_t N, bits, passes; };
static const WidthCase widths[] = {
    {1, 1, 1}, {200, 8, 1}, {255, 8, 1}, {256, 9, 2}, {300, 9, 2}, {65535, 16, 2}, {65536, 17, 3}, {70000, 17, 3},
    {(1 << 24) - 1, 24, 3}, {1 << 24, 25, 4}, {(1 << 24) + 3, 25, 4}, {2147483647, 31, 4},
};

int main()
{
    int bad = 0, n = 0;
    for (const WidthCase& c : widths) {
        n++;
        if (update_bits(c.N) != c.bits || update_passes(c.N) != c.passes) {
            printf("MISMATCH N %d: bits %d passes %d, want %d %d\n", c.N, update_bits(c.N), update_passes(c.N), c.bits, c.passes);
            bad++;
        }
    }
    printf("%d cases, %d failed\n", n, bad);
    return bad ? 1 : 0;
}
