/* y2_bf16_rn and y2_split3 of include/y2_split_rule.h on bit patterns: reads uint32 patterns from argv[1], writes per
 * pattern four uint16 -- bf16_rn, h, m, l -- to argv[2].  tests/test_train_precision_host.py compares them with the numpy
 * restatement of tests/train_bf16_rule.py. */
#include <stdio.h>
#include <stdlib.h>
#include "y2_split_rule.h"

int main(int argc, char **argv)
{
    FILE *in, *out;
    uint32_t u;
    if (argc != 3 || !(in = fopen(argv[1], "rb")) || !(out = fopen(argv[2], "wb"))) return 2;
    while (fread(&u, sizeof u, 1, in) == 1) {
        uint16_t r[4];
        const float a = y2_bits_f32(u);
        r[0] = y2_bf16_rn(a);
        y2_split3(a, &r[1], &r[2], &r[3]);
        if (fwrite(r, sizeof r, 1, out) != 1) return 3;
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 3;
}
