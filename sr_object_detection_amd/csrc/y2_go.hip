// Go on the device (include/y2_hip.h y2h_go_*): the eight board views and their merge (go.c:262-289 predict_move), the
// rules (calculate_liberties :188, move_go :304, suicide_go :326, legal_go :338), the decision of generate_move from
// :362 on, and the record decoder of valid_go / random_go_moves.  Boards are [n][361] floats holding exactly 0, 1 or -1,
// row-major -- the network's 19x19x1 input, where NHWC and NCHW coincide.
//
// The rules run one workgroup per position, one thread per point.  Board, group labels and the per-group counters live in
// LDS.  Groups come from label propagation with pointer jumping: every stone starts as its own label and takes the
// smallest label among itself, its same-coloured neighbours and its label's label until nothing moves -- the fixed
// point is the smallest point index of each group whatever order the threads ran in.  A group's liberty count is one
// LDS integer add per (empty point, distinct adjacent group); legal_go's 91-byte comparison with `ko` becomes a count
// of points at which the board after the move differs from the ko board: the number before the move, corrected at the
// played point and by two per-group sums for every captured group.  Integers only, no global atomics: the same bytes
// on every run.
#include "y2_common.hpp"

namespace {

constexpr int GO_P = 361, GO_T = 384, GO_KO = 91, GO_REC = 93;

// rotate_image_cw (image.c:1035-1054), read from its assignments: one turn is new[r][c] = old[c][18-r].  The source
// point of (r, c) after k turns:
__device__ __forceinline__ int go_src(int k, int r, int c)
{
    switch (k & 3) {
    case 0: return r * 19 + c;
    case 1: return c * 19 + (18 - r);
    case 2: return (18 - r) * 19 + (18 - c);
    default: return (18 - c) * 19 + r;
    }
}

// view v of a board: rotate_image_cw(board, v), then flip_image (columns mirrored, image.c:1056) when v >= 4
__device__ __forceinline__ int go_view_src(int v, int p)
{
    const int r = p / 19, c = p - r * 19;
    return go_src(v, r, v >= 4 ? 18 - c : c);
}

// the way back for an output row: un-flip when v >= 4, then rotate_image_cw(-v) (go.c:276-277)
__device__ __forceinline__ int go_unview_src(int v, int p)
{
    const int r = p / 19, c = p - r * 19;
    const int s = go_src(4 - (v & 3), r, c), sr = s / 19, sc = s - sr * 19;
    return sr * 19 + (v >= 4 ? 18 - sc : sc);
}

__global__ __launch_bounds__(256) void go_views_kernel(const float *boards, const int *players, int n, int views, float *x)
{
    const long total = (long)n * views * GO_P;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int row = (int)(idx / GO_P), p = (int)(idx - (long)row * GO_P);
        const int b = row / views, v = row - b * views;
        const float val = boards[(size_t)b * GO_P + go_view_src(v, p)];
        x[idx] = players[b] < 0 ? -val : val;                   // flip_board (go.c:357)
    }
}

__global__ __launch_bounds__(256) void go_merge_kernel(const float *rows, int ld, const float *boards, int n, int views, float *move)
{
    const long total = (long)n * GO_P;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int b = (int)(idx / GO_P), p = (int)(idx - (long)b * GO_P);
        const float *r0 = rows + (size_t)b * views * ld;
        float acc = r0[p];                                      // copy_cpu
        if (views > 1) {
            for (int v = 1; v < 8; ++v) acc = acc + r0[(size_t)v * ld + go_unview_src(v, p)];      // axpy_cpu, views in order
            acc = acc * 0.125f;                                 // scal_cpu(1./8.)
        }
        move[idx] = boards[idx] != 0.f ? 0.f : acc;             // go.c:286-288 (the sign of the player flip does not matter)
    }
}

// ---- the rules ----
struct go_lds {
    int label[GO_P];        // stones: the group's smallest point index; empty points: -1
    int cnt[GO_P];          // by label: the group's liberties
    int flag;
    signed char b[GO_P];
};

__device__ __forceinline__ int go_sign(float v) { return v > 0.f ? 1 : v < 0.f ? -1 : 0; }

// the up to four neighbours of point t as point indices, -1 off the board
__device__ __forceinline__ void go_nbrs(int t, int q[4])
{
    const int r = t / 19, c = t - r * 19;
    q[0] = r < 18 ? t + 19 : -1;
    q[1] = r > 0 ? t - 19 : -1;
    q[2] = c < 18 ? t + 1 : -1;
    q[3] = c > 0 ? t - 1 : -1;
}

// labels and liberty counts of the board in L.b; called by all GO_T threads, ends behind a barrier
__device__ void go_groups(go_lds &L, int t)
{
    const bool on = t < GO_P;
    const int col = on ? L.b[t] : 0;
    int q[4] = { -1, -1, -1, -1 };
    if (on) { go_nbrs(t, q); L.label[t] = col ? t : -1; L.cnt[t] = 0; }
    if (t == 0) L.flag = 0;
    __syncthreads();
    for (;;) {
        int best = -1;
        if (col) {
            best = L.label[t];
            for (int k = 0; k < 4; ++k)
                if (q[k] >= 0 && L.b[q[k]] == col) { const int o = L.label[q[k]]; best = o < best ? o : best; }
            const int up = L.label[best];                       // pointer jumping: the label's own label
            best = up < best ? up : best;
        }
        __syncthreads();                                        // every read of this round is done
        if (col && best < L.label[t]) { L.label[t] = best; L.flag = 1; }
        __syncthreads();
        const int moved = L.flag;
        __syncthreads();
        if (!moved) break;
        if (t == 0) L.flag = 0;
        __syncthreads();
    }
    // calculate_liberties: an empty point adds one to each DISTINCT adjacent group (the per-point `visited`, go.c:195)
    if (on && !col) {
        int g[4];
        for (int k = 0; k < 4; ++k) g[k] = (q[k] >= 0 && L.b[q[k]]) ? L.label[q[k]] : -1;
        for (int k = 0; k < 4; ++k) {
            bool seen = g[k] < 0;
            for (int j = 0; j < k; ++j) seen = seen || g[j] == g[k];
            if (!seen) atomicAdd(&L.cnt[g[k]], 1);
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int go_lib(const go_lds &L, int p) { return L.b[p] ? L.cnt[L.label[p]] : 0; }

// move_go on the board in L.b with the labels and counts taken BEFORE the stone was placed: every adjacent opposing group
// whose count is 1 goes (remove_connected, go.c:291-301: all stones of a group carry one count, so a group goes whole).
// Called by all threads behind go_groups; ends behind a barrier.
__device__ void go_place(go_lds &L, int t, int mv, int pl)
{
    int q[4], dead[4];
    go_nbrs(mv, q);
    for (int k = 0; k < 4; ++k) dead[k] = (q[k] >= 0 && L.b[q[k]] && L.b[q[k]] == -pl && L.cnt[L.label[q[k]]] == 1) ? L.label[q[k]] : -1;
    bool gone = false;
    if (t < GO_P && t != mv && L.b[t] == -pl) {
        const int g = L.label[t];
        gone = g == dead[0] || g == dead[1] || g == dead[2] || g == dead[3];
    }
    __syncthreads();
    if (gone) L.b[t] = 0;
    if (t == mv) L.b[t] = (signed char)pl;
    __syncthreads();
}

// board_to_string (go.c:75-90): byte i holds points 4i..4i+3, bit 2j = (value == 1), bit 2j+1 = (value == -1)
__device__ __forceinline__ unsigned char go_pack_byte(const go_lds &L, int i, int sign)
{
    unsigned v = 0;
    for (int j = 0; j < 4; ++j) {
        const int p = 4 * i + j;
        if (p >= GO_P) break;
        const int s = L.b[p] * sign;
        if (s == 1) v |= 1u << (2 * j);
        if (s == -1) v |= 2u << (2 * j);
    }
    return (unsigned char)v;
}

__global__ __launch_bounds__(GO_T) void go_rules_kernel(const float *boards, const unsigned char *ko, const int *players,
                                                        int *liberties, unsigned char *legal, unsigned char *suicide)
{
    __shared__ go_lds L;
    __shared__ signed char kob[GO_P];
    __shared__ int mm[GO_P], nz[GO_P];      // by label: stones that differ from the ko board / that the ko board has a stone under
    __shared__ int diff0, kobad;
    const int b = blockIdx.x, t = threadIdx.x, pl = players[b];
    const bool on = t < GO_P;
    if (on) {
        L.b[t] = (signed char)go_sign(boards[(size_t)b * GO_P + t]);
        const unsigned byte = ko ? ko[(size_t)b * GO_KO + (t >> 2)] : 0u;
        const unsigned two = (byte >> (2 * (t & 3))) & 3u;
        kob[t] = two == 1 ? 1 : two == 2 ? -1 : two == 3 ? 2 : 0;    // both bits set: no board packs to that
        mm[t] = 0; nz[t] = 0;
    }
    if (t == 0) { diff0 = 0; kobad = ko ? (ko[(size_t)b * GO_KO + 90] >> 2) != 0 : 0; }
    go_groups(L, t);
    if (on) {
        const int differs = L.b[t] != kob[t];
        if (differs) atomicAdd(&diff0, 1);
        if (L.b[t]) {
            if (differs) atomicAdd(&mm[L.label[t]], 1);
            if (kob[t]) atomicAdd(&nz[L.label[t]], 1);
        }
    }
    __syncthreads();
    if (!on) return;
    int q[4];
    go_nbrs(t, q);
    if (liberties) liberties[(size_t)b * GO_P + t] = go_lib(L, t);
    if (legal) {
        int ok = 0;
        if (!L.b[t]) {
            // points at which the board after the move differs from the ko board: zero means memcmp(next, ko, 91) == 0
            int d = diff0 - (kob[t] != 0) + (kob[t] != pl);
            int g[4];
            for (int k = 0; k < 4; ++k) {
                g[k] = (q[k] >= 0 && L.b[q[k]] && L.b[q[k]] == -pl && L.cnt[L.label[q[k]]] == 1) ? L.label[q[k]] : -1;
                bool seen = g[k] < 0;
                for (int j = 0; j < k; ++j) seen = seen || g[j] == g[k];
                if (!seen) d += nz[g[k]] - mm[g[k]];
            }
            ok = kobad || d != 0;
        }
        legal[(size_t)b * GO_P + t] = (unsigned char)ok;
    }
    if (suicide) {
        int safe = 0;                                           // makes_safe_go (go.c:315-324) on the four neighbours
        for (int k = 0; k < 4; ++k) {
            if (q[k] < 0) continue;
            const int v = L.b[q[k]], lq = go_lib(L, q[k]);
            safe |= v == -pl ? lq <= 1 : v == 0 ? 1 : lq > 1;
        }
        suicide[(size_t)b * GO_P + t] = (unsigned char)!safe;
    }
}

// move_go + board_to_string per position; a moves[b] outside 0..360 leaves the board as it is (it is still packed)
__global__ __launch_bounds__(GO_T) void go_apply_kernel(float *boards, const int *players, const int *moves, unsigned char *strings)
{
    __shared__ go_lds L;
    const int b = blockIdx.x, t = threadIdx.x, pl = players[b], mv = moves[b];
    if (t < GO_P) L.b[t] = (signed char)go_sign(boards[(size_t)b * GO_P + t]);
    __syncthreads();
    if (mv >= 0 && mv < GO_P) {
        go_groups(L, t);
        go_place(L, t, mv, pl);
        if (t < GO_P) boards[(size_t)b * GO_P + t] = (float)L.b[t];
    }
    if (strings && t < GO_KO) strings[(size_t)b * GO_KO + t] = go_pack_byte(L, t, 1);
}

// one ply of self_go's loop (go.c:801-822) for every game still alive: a -1 ends the game; otherwise the record (row,
// column, the board packed from the mover's side) is written, the move is made and the new board is packed into ko[b]
__global__ __launch_bounds__(GO_T) void go_play_kernel(float *boards, unsigned char *ko, int player, const int *index,
                                                       int *alive, unsigned char *records, int *counts, int max_moves)
{
    __shared__ go_lds L;
    const int b = blockIdx.x, t = threadIdx.x;
    const int live = alive[b], mv = index[b], cnt = counts[b];
    __syncthreads();                                            // every thread has read alive and counts
    if (!live) return;
    if (mv < 0 || mv >= GO_P || cnt >= max_moves) { if (t == 0) alive[b] = 0; return; }
    if (t < GO_P) L.b[t] = (signed char)go_sign(boards[(size_t)b * GO_P + t]);
    __syncthreads();
    unsigned char *rec = records + ((size_t)b * max_moves + cnt) * GO_REC;
    if (t == 0) { rec[0] = (unsigned char)(mv / 19); rec[1] = (unsigned char)(mv % 19); counts[b] = cnt + 1; }
    if (t < GO_KO) rec[2 + t] = go_pack_byte(L, t, player);     // flip_board around board_to_string (go.c:812-816)
    go_groups(L, t);
    go_place(L, t, mv, player);
    if (t < GO_P) boards[(size_t)b * GO_P + t] = (float)L.b[t];
    if (t < GO_KO) ko[(size_t)b * GO_KO + t] = go_pack_byte(L, t, 1);
}

// generate_move from go.c:362 on.  The sequential parts (top_k's insertion, max_index, sample_array's sum and
// subtraction) run on one lane: their order decides the result.
__global__ __launch_bounds__(GO_T) void go_pick_kernel(const float *move, int ld, const unsigned char *legal, const unsigned char *suicide,
                                                       float thresh, const float *u, int *index, float *kept)
{
    __shared__ float a[GO_P];
    __shared__ float cut;
    const int b = blockIdx.x, t = threadIdx.x;
    if (t < GO_P) a[t] = legal[(size_t)b * GO_P + t] ? move[(size_t)b * ld + t] : 0.f;
    __syncthreads();
    if (t == 0) {
        // top_k(move, 361, 5) (utils.c:179-193): strict >, a displaced entry moves on down the list
        int ti[5] = { -1, -1, -1, -1, -1 };
        float tv[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
        for (int i = 0; i < GO_P; ++i) {
            int ci = i;
            float cv = a[i];
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (ti[j] < 0 || cv > tv[j]) {
                    const int si = ci; const float sv = cv;
                    ci = ti[j]; cv = tv[j];
                    ti[j] = si; tv[j] = sv;
                }
            }
        }
        cut = thresh > tv[0] ? tv[4] : thresh;                  // go.c:370
    }
    __syncthreads();
    if (t < GO_P) {
        if (a[t] < cut) a[t] = 0.f;
        if (kept) kept[(size_t)b * GO_P + t] = a[t];
    }
    __syncthreads();
    if (t != 0) return;
    int mx = 0;                                                 // max_index (utils.c:533): the first maximum
    float best = a[0];
    for (int i = 1; i < GO_P; ++i) if (a[i] > best) { best = a[i]; mx = i; }
    float sum = 0.f;                                            // sample_array (utils.c:520-531)
    for (int i = 0; i < GO_P; ++i) sum += a[i];
    const float scale = (float)(1. / (double)sum);
    float r = u[b];
    int c = GO_P - 1;
    for (int i = 0; i < GO_P; ++i) {
        const float v = a[i] * scale;
        r = r - v;
        if (r <= 0.f) { c = i; break; }
    }
    const unsigned char *su = suicide + (size_t)b * GO_P;
    index[b] = su[mx] ? -1 : su[c] ? mx : c;                    // go.c:395-399
}

// max_index of each row: the first maximum
__global__ __launch_bounds__(64) void go_argmax_kernel(const float *move, int ld, int n, int *index)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const float *a = move + (size_t)b * ld;
    int mx = 0;
    float best = a[0];
    for (int i = 1; i < GO_P; ++i) if (a[i] > best) { best = a[i]; mx = i; }
    index[b] = mx;
}

// item i of a batch from record pick[i] (or i): string_to_board (go.c:56-73) of bytes 2..92.  With labels: the one-hot
// label at (row, col), the board cleared there, flip_image when flip[i], then rotate_image_cw(rot[i]) on both
// (random_go_moves, go.c:96-114) -- flip first, the opposite of predict_move's views.
__global__ __launch_bounds__(GO_T) void go_decode_kernel(const unsigned char *records, const int *pick, const int *flip, const int *rot,
                                                         float *boards, float *labels)
{
    const int i = blockIdx.x, t = threadIdx.x;
    if (t >= GO_P) return;
    const unsigned char *rec = records + (size_t)(pick ? pick[i] : i) * GO_REC;
    int s = t;
    if (labels) {
        const int r = t / 19, c = t - r * 19;
        s = go_src(rot ? rot[i] : 0, r, c);
        if (flip && flip[i]) { const int sr = s / 19, sc = s - sr * 19; s = sr * 19 + 18 - sc; }
    }
    const unsigned two = (rec[2 + (s >> 2)] >> (2 * (s & 3))) & 3u;
    float v = (two & 1u) ? 1.f : (two & 2u) ? -1.f : 0.f;
    if (labels) {
        const int at = (int)(signed char)rec[0] * 19 + (int)(signed char)rec[1];
        if (s == at) v = 0.f;                                   // go.c:102
        labels[(size_t)i * GO_P + t] = s == at ? 1.f : 0.f;
    }
    boards[(size_t)i * GO_P + t] = v;
}

}  // namespace

extern "C" int y2h_go_views(const float *boards, const int *players, int n, int multi, float *x, y2h_stream s)
{
    if (!boards || !players || !x || n <= 0) return Y2H_EINVAL;
    const int views = multi ? 8 : 1;
    hipLaunchKernelGGL(go_views_kernel, dim3(y2h_grid((long)n * views * GO_P, 256)), dim3(256), 0, S(s), boards, players, n, views, x);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_merge(const float *rows, int ld, const float *boards, int n, int multi, float *move, y2h_stream s)
{
    if (!rows || !boards || !move || n <= 0 || ld < GO_P) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_merge_kernel, dim3(y2h_grid((long)n * GO_P, 256)), dim3(256), 0, S(s), rows, ld, boards, n, multi ? 8 : 1, move);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_rules(const float *boards, const unsigned char *ko, const int *players, int n, int *liberties,
                            unsigned char *legal, unsigned char *suicide, y2h_stream s)
{
    if (!boards || !players || n <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_rules_kernel, dim3((unsigned)n), dim3(GO_T), 0, S(s), boards, ko, players, liberties, legal, suicide);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_apply(float *boards, const int *players, const int *moves, int n, unsigned char *strings, y2h_stream s)
{
    if (!boards || !players || !moves || n <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_apply_kernel, dim3((unsigned)n), dim3(GO_T), 0, S(s), boards, players, moves, strings);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_play(float *boards, unsigned char *ko, int player, const int *index, int *alive,
                           unsigned char *records, int *counts, int max_moves, int n, y2h_stream s)
{
    if (!boards || !ko || !index || !alive || !records || !counts || n <= 0 || max_moves <= 0 || (player != 1 && player != -1))
        return Y2H_EINVAL;
    hipLaunchKernelGGL(go_play_kernel, dim3((unsigned)n), dim3(GO_T), 0, S(s), boards, ko, player, index, alive, records, counts,
                       max_moves);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_pick(const float *move, int ld, const unsigned char *legal, const unsigned char *suicide, int n, float thresh,
                           const float *u, int *index, float *kept, y2h_stream s)
{
    if (!move || !legal || !suicide || !u || !index || n <= 0 || ld < GO_P) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_pick_kernel, dim3((unsigned)n), dim3(GO_T), 0, S(s), move, ld, legal, suicide, thresh, u, index, kept);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_argmax(const float *move, int ld, int n, int *index, y2h_stream s)
{
    if (!move || !index || n <= 0 || ld < GO_P) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_argmax_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, S(s), move, ld, n, index);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}

extern "C" int y2h_go_decode(const unsigned char *records, const int *pick, const int *flip, const int *rot, int n, float *boards,
                             float *labels, y2h_stream s)
{
    if (!records || !boards || n <= 0) return Y2H_EINVAL;
    hipLaunchKernelGGL(go_decode_kernel, dim3((unsigned)n), dim3(GO_T), 0, S(s), records, pick, flip, rot, boards, labels);
    Y2H_LAUNCH_CHECK();
    return Y2H_OK;
}
