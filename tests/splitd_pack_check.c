/* Stand-alone driver of the direct split form's filter packer (include/y2_splitd_rule.h) for tests/test_splitd_rule_cpu.py:
 *     splitd_pack_check <c> <n> <bn> <file>
 * packs the reference-layout weights w[i] = ((i * 2654435761 + 12345) >> 3 & 0xffffff) / 2^24 - 1/2 and writes the slot. */
#include <stdio.h>
#include <stdlib.h>

#include "y2_splitd_rule.h"

int main(int argc, char **argv)
{
    int c, n, bn;
    size_t i, count, elems;
    float *w;
    uint16_t *up;
    FILE *f;
    if (argc != 5) return 2;
    c = atoi(argv[1]); n = atoi(argv[2]); bn = atoi(argv[3]);
    if (c <= 0 || c % Y2_SPLIT_BK || n <= 0 || (bn != 128 && bn != 256)) return 2;
    count = (size_t)n * c * 9;
    elems = y2_splitd_u_elems(n, c, bn);
    w = malloc(count * sizeof *w);
    up = malloc(elems * sizeof *up);
    if (!w || !up) return 3;
    for (i = 0; i < count; ++i)
        w[i] = (float)((double)((((uint64_t)i * 2654435761u + 12345u) >> 3) & 0xffffffu) / 16777216.0 - 0.5);
    y2_splitd_pack_u(up, w, n, c, bn);
    f = fopen(argv[4], "wb");
    if (!f || fwrite(up, sizeof *up, elems, f) != elems) return 4;
    fclose(f);
    free(w); free(up);
    return 0;
}
