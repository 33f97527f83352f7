/*
 * The stream-K share rule.  conv_mfma_kernel's stream-K form takes its share from y2_sk_share_of; the launches that add
 * the pieces up (sk_reduce_kernel, conv_p8_fixup_kernel) start at y2_sk_first and go by y2_sk_walk.  conv_p8_f16_kernel
 * still writes y2_sk_share_of out on y2_sk_begin (its comment says why).  Plain integer arithmetic, host and device alike.
 *
 * `tiles` output tiles of `nk` K-steps each are I = tiles * nk K-steps in tile-major order.  Workgroup w of G owns the
 * K-steps [w * I / G, (w + 1) * I / G).
 *
 * PRECONDITION: 1 <= tiles <= G and nk >= 1 (y2_sk_fits).  Then a share is never longer than one tile, so it is empty,
 * one piece (tile, [kb0, ke0)), or that piece up to the end of its tile plus the head [0, ke1) of the next tile.
 *
 * Slots are the callers' business: 2 * w + piece, both pieces of a share stored (conv_mfma_kernel's stream-K form,
 * conv_p8_f16_kernel).
 */
#ifndef Y2_STREAMK_RULE_H
#define Y2_STREAMK_RULE_H

#ifndef Y2_HD
#ifdef __HIPCC__
#define Y2_HD __host__ __device__ static inline
#else
#define Y2_HD static inline
#endif
#endif

Y2_HD int y2_sk_fits(long tiles, int nk, long G) { return tiles >= 1 && nk >= 1 && tiles <= G; }

/* first K-step of workgroup w's share (w = G: one past the last K-step) */
Y2_HD long y2_sk_begin(long w, long I, long G) { return w * I / G; }

typedef struct {
    int n;          /* pieces: 0 (empty share, exactly when its two bounds are equal), 1 or 2 */
    int tile;       /* piece 0 is K-steps [kb0, ke0) of this tile, */
    int kb0, ke0;
    int ke1;        /* piece 1 (n == 2) is K-steps [0, ke1) of tile + 1 */
} y2_sk_share;

Y2_HD y2_sk_share y2_sk_share_of(long w, long tiles, int nk, long G)
{
    y2_sk_share s = {0, 0, 0, 0, 0};
    const long I = tiles * nk;
    const long lo = y2_sk_begin(w, I, G), hi = y2_sk_begin(w + 1, I, G);
    if (hi > lo) {
        const int t0 = (int)(lo / nk), k0 = (int)(lo - (long)t0 * nk), len = (int)(hi - lo);
        s.tile = t0; s.kb0 = k0; s.ke0 = k0 + len < nk ? k0 + len : nk; s.n = 1;
        if (k0 + len > nk) { s.ke1 = k0 + len - nk; s.n = 2; }
    }
    return s;
}

/* the first share that reaches into `tile`: the one that holds the tile's K-step 0 */
Y2_HD long y2_sk_first(long tile, long tiles, int nk, long G)
{
    const long I = tiles * nk, tb = tile * nk;
    long w = tb * G / I;
    while (w > 0 && y2_sk_begin(w, I, G) > tb) --w;
    while (w + 1 < G && y2_sk_begin(w + 1, I, G) <= tb) ++w;
    return w;
}

/* The walk over the shares of `tile` in ascending K:
 *     for (w = y2_sk_first(tile, ...); y2_sk_walk(&w, &piece, tile, ...); ++w)  ... share w, its piece `piece` ...
 * Moves *w past empty shares; 0 when no further share reaches into the tile.  *piece = 1 when the share began in the
 * previous tile (what it holds of this one is its second piece). */
Y2_HD int y2_sk_walk(long *w, int *piece, long tile, long tiles, int nk, long G)
{
    const long I = tiles * nk, tb = tile * nk, te = tb + nk;
    for (; *w < G; ++*w) {
        const long lo = y2_sk_begin(*w, I, G), hi = y2_sk_begin(*w + 1, I, G);
        if (lo >= te) return 0;
        if (hi <= lo) continue;
        *piece = lo < tb ? 1 : 0;
        return 1;
    }
    return 0;
}

#endif
