/* Stand-alone check of include/y2_split_rule.h (tests/test_wino_split_cpu.py compiles and runs it, once more under
 * -fsanitize=address,undefined).
 *     wino_split_check split            the 3-way split over random and special floats; prints "ok <count>"
 *     wino_split_check pack C N FILE    y2_split_pack_u of the test weights w(i) below, raw bf16 values to FILE */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "y2_split_rule.h"

static unsigned long long g_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32(void)
{
    g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

static long g_count = 0;

static int sig_bits(float a)          /* significant bits of a finite non-zero value */
{
    uint32_t u = y2_f32_bits(a), man = u & 0x7fffffu;
    int n = 24, e = (int)(u >> 23 & 0xff);
    if (e == 0) { n = 0; while (man >> n) ++n; }          /* subnormal: no hidden bit */
    else man |= 0x800000u;
    while (n > 0 && !(man & 1u)) { man >>= 1; --n; }
    return n;
}

static int check(float a)
{
    uint16_t h, m, l;
    const uint32_t mag = y2_f32_bits(a) & 0x7fffffffu;
    ++g_count;
    y2_split3(a, &h, &m, &l);
    if (mag >= 0x7f800000u) {          /* the non-finite rule */
        if (m != 0 || l != 0) { printf("non-finite %08x: m %04x l %04x\n", y2_f32_bits(a), m, l); return 1; }
        if (mag == 0x7f800000u && y2_f32_bits(y2_bf16_f32(h)) != y2_f32_bits(a)) { printf("inf %08x: h %04x\n", y2_f32_bits(a), h); return 1; }
        if (mag > 0x7f800000u && !isnan(y2_bf16_f32(h))) { printf("nan %08x: h %04x\n", y2_f32_bits(a), h); return 1; }
        return 0;
    }
    {
        /* every bit of a at or above 2^-133, the smallest bf16 subnormal, can be carried: all normal values from 2^-110 up, and
         * the subnormals and tiny values that are multiples of 2^-133.  Then h + m + l == a bit for bit (the sum is taken
         * smallest first, each step exact) and l is the exact second remainder, a bf16 value.  Below that the parts are the
         * nearest bf16 values and the sum is within half of 2^-133. */
        const double scaled = ldexp((double)a, 133);
        const float s = (y2_bf16_f32(l) + y2_bf16_f32(m)) + y2_bf16_f32(h);
        if (scaled == floor(scaled)) {
            if (a == 0.f ? s != 0.f : y2_f32_bits(s) != y2_f32_bits(a)) { printf("%08x: %04x + %04x + %04x = %08x\n", y2_f32_bits(a), h, m, l, y2_f32_bits(s)); return 1; }
            if (y2_f32_bits((a - y2_bf16_f32(h)) - y2_bf16_f32(m)) != (uint32_t)l << 16) { printf("%08x: l is not a bf16 value\n", y2_f32_bits(a)); return 1; }
        } else if (fabs((double)a - (double)s) > ldexp(1.0, -134)) { printf("%08x: off by more than 2^-134\n", y2_f32_bits(a)); return 1; }
        if (isinf(y2_bf16_f32(h)) || isinf(y2_bf16_f32(m))) { printf("%08x: a part is infinite\n", y2_f32_bits(a)); return 1; }
        if (scaled == floor(scaled) && a != 0.f && sig_bits(a) <= 16 && (l & 0x7fffu) != 0) { printf("%08x has %d significant bits, l %04x\n", y2_f32_bits(a), sig_bits(a), l); return 1; }
    }
    return 0;
}

static int run_split(void)
{
    static const uint32_t special[] = { 0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x00800000u, 0x00012345u, 0x807fffffu,
                                        0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00001u, 0x7f800001u, 0x7f7fffffu, 0xff7fffffu, 0x7f7f8000u,
                                        0x7f7f7fffu, 0x3f800000u, 0x3f7fffffu, 0x3f808000u, 0x3f818000u, 0x3f80ffffu };
    long i;
    int bad = 0;
    for (i = 0; i < (long)(sizeof special / sizeof special[0]); ++i) bad |= check(y2_bits_f32(special[i]));
    bad |= check(FLT_MAX); bad |= check(-FLT_MAX); bad |= check(FLT_MIN);
    for (i = 0; i < 1500000 && !bad; ++i) bad |= check(y2_bits_f32(rnd32()));                        /* every exponent, subnormals and non-finites included */
    for (i = 0; i < 500000 && !bad; ++i) bad |= check(ldexpf((float)(rnd32() & 0xffffffu), (int)(rnd32() % 59) - 53));      /* 2^-29 .. 2^29 */
    for (i = 0; i <= (1 << 24) && !bad; i += (i < 70000 ? 1 : 251)) { bad |= check((float)i); bad |= check(-(float)i); }  /* integers up to 2^24 */
    bad |= check(16777216.f);
    for (i = 0; i < 300000 && !bad; ++i) bad |= check(ldexpf((float)(rnd32() & 0xffffu), (int)(rnd32() % 80) - 40));        /* <= 16 significant bits */
    for (i = -(1 << 17); i <= (1 << 17) && !bad; ++i) bad |= check((float)i * 0.25f);                                     /* multiples of 1/4 */
    if (bad) return 1;
    printf("ok %ld\n", g_count);
    return 0;
}

/* weight i of the pack test: a 24-bit dyadic fraction in [-0.5, 0.5), so G g G^T is exact in double and all three planes are used */
static float test_weight(size_t i)
{
    const uint32_t v = (uint32_t)((i * 2654435761ull + 12345u) >> 3) & 0xffffffu;
    return (float)v / 16777216.f - 0.5f;
}

static int run_pack(int c, int n, const char *path)
{
    const size_t nw = (size_t)n * c * 9, bytes = y2_split_bytes(y2_split_rows_pad(n), c);
    float *w = malloc(nw * sizeof(float));
    uint16_t *u = malloc(bytes);
    FILE *f;
    size_t i;
    if (!w || !u) return 1;
    for (i = 0; i < nw; ++i) w[i] = test_weight(i);
    y2_split_pack_u(u, w, n, c);
    f = fopen(path, "wb");
    if (!f || fwrite(u, 1, bytes, f) != bytes) return 1;
    fclose(f);
    free(w); free(u);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "split")) return run_split();
    if (argc == 5 && !strcmp(argv[1], "pack")) return run_pack(atoi(argv[2]), atoi(argv[3]), argv[4]);
    fprintf(stderr, "usage: %s split | pack C N FILE\n", argv[0]);
    return 2;
}
