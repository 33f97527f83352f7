/*
 * y2_hip.h -- the thin C-ABI device layer of the MI355X (gfx950) YOLOv2 engine.
 *
 * Everything the C host code (csrc/host, C sources) needs from the GPU goes through
 * these entry points: plain pointers and sizes, no C++ or torch types.  It
 * replaces the reference's device wrapper and its per-layer *_gpu functions:
 *
 *   device/memory      src_yolo2/cuda.h:24-33  (cuda_set_device, cuda_make_array,
 *                      cuda_push_array, cuda_pull_array, cuda_free, check_error)
 *   conv+BN+bias+act   src_yolo2/convolutional_kernels.cu:77-131
 *                      (fill + im2col_ongpu + gemm_ongpu + normalize_gpu +
 *                       scale_bias_gpu + add_bias_gpu + activate_array_ongpu,
 *                       >= 6 launches per layer there; ONE launch here)
 *   maxpool            src_yolo2/maxpool_layer_kernels.cu:87-97
 *   reorg              src_yolo2/reorg_layer.c:97-104 (reorg_ongpu, blas_kernels.cu:332)
 *   route              src_yolo2/route_layer.c:104-117 (copy_ongpu per input per item)
 *   region head        src_yolo2/region_layer.c:383-417 (flatten_ongpu + softmax_gpu,
 *                      then D2H and logistic on the CPU there; all on device here)
 *   decode / NMS       src_yolo2/region_layer.c:328-379, src_yolo2/box.c:249-277
 *                      (CPU-only in the reference, both builds)
 *   avgpool / softmax  src_yolo2/avgpool_layer_kernels.cu:44, src_yolo2/softmax_layer.c:73
 *
 * Data layout: activations are NHWC fp32 with an explicit channel stride
 * (`ld`, in floats) so that [route] concatenation is a channel-offset write
 * instead of a copy.  Convolution weights are pre-packed per layer as
 * [Cout][kh][kw][Cin] (K index = (kh*size + kw)*Cin + ci).
 *
 * All functions return 0 on success or a negative Y2H_E* code; none aborts.
 * The legacy abort-on-error contract (cuda.c:27-49 check_error) is applied one
 * level up, in the host C layer.
 */
#ifndef Y2_HIP_H
#define Y2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Y2H_OK            0
#define Y2H_EHIP         -1   /* a HIP runtime call failed (y2h_last_error() has the text) */
#define Y2H_EINVAL       -2   /* argument outside what the kernels support */
#define Y2H_ENODEV       -3   /* no gfx950 device visible */

typedef void *y2h_stream;   /* hipStream_t */
typedef void *y2h_event;    /* hipEvent_t */
typedef void *y2h_graph;    /* hipGraphExec_t */

/* activation codes (src_yolo2/activations.h:7).  0-3 are the ones the target cfgs use and every kernel's epilogue
 * applies in place; the others only exist as the separate pass y2h_activate_array (the engine then runs the
 * producing kernel with Y2H_ACT_LINEAR, which is exactly the reference's own order: activate_array is a pass of its
 * own over the stored fp32 output, activations.c:95-101) */
enum { Y2H_ACT_LINEAR = 0, Y2H_ACT_LEAKY = 1, Y2H_ACT_LOGISTIC = 2, Y2H_ACT_RELU = 3,
       Y2H_ACT_RELIE = 4, Y2H_ACT_RAMP = 5, Y2H_ACT_TANH = 6, Y2H_ACT_PLSE = 7, Y2H_ACT_ELU = 8, Y2H_ACT_LOGGY = 9,
       Y2H_ACT_STAIR = 10, Y2H_ACT_HARDTAN = 11, Y2H_ACT_LHTAN = 12 };

/* ---- device / memory / streams (cuda.h:24-33) ---- */
int         y2h_device_count(void);
int         y2h_set_device(int dev);
int         y2h_get_device(int *dev);
const char *y2h_last_error(void);
const char *y2h_device_name(void);
/* PCI address ("0000:c1:00.0") of device `dev` (< 0: the current one), "" if unknown: lets a launcher pin a rank's host
 * threads to the NUMA node of its GPU (/sys/bus/pci/devices/<address>/numa_node) */
const char *y2h_device_pci_bus_id(int dev);
int         y2h_malloc(void **ptr, size_t bytes);
int         y2h_free(void *ptr);
int         y2h_host_alloc(void **ptr, size_t bytes);           /* pinned host memory */
int         y2h_host_free(void *ptr);
/* pin an existing host allocation.  HAZARD (profiles/r02_notes.md): only register buffers that own their pages -- mmap'ed
 * or page-aligned AND page-padded.  A registered range that ends inside a heap page makes the runtime treat a pageable
 * buffer that malloc placed in the rest of that page as pinned: an asynchronous copy from it then faults on the GPU.
 * The engine itself never registers memory (its staging buffers come from y2h_host_alloc). */
int         y2h_host_register(void *ptr, size_t bytes);
int         y2h_host_unregister(void *ptr);
int         y2h_memcpy_h2d(void *dst, const void *src, size_t bytes, y2h_stream s);
int         y2h_memcpy_d2h(void *dst, const void *src, size_t bytes, y2h_stream s);
unsigned long y2h_d2h_copies(void);      /* y2h_memcpy_d2h calls of this process that moved bytes */
unsigned long y2h_stream_syncs(void);    /* y2h_stream_sync calls of this process: the host waits a test may count */
int         y2h_memcpy_d2d(void *dst, const void *src, size_t bytes, y2h_stream s);
int         y2h_memset(void *dst, int value, size_t bytes, y2h_stream s);
int         y2h_stream_create(y2h_stream *s);
int         y2h_stream_destroy(y2h_stream s);
int         y2h_stream_sync(y2h_stream s);
int         y2h_device_sync(void);
/* the clock (GHz) this device holds under a full-chip fp32 matrix load: `iters` x 2 v_mfma_f32_32x32x2_f32 per wave on
 * every CU, in-kernel s_memtime / s_memrealtime stamps, median over waves (diagnostic: benchmark lines quote it) */
int         y2h_clock_probe(int iters, float *ghz, y2h_stream s);
int         y2h_event_create(y2h_event *e);
int         y2h_event_destroy(y2h_event e);
int         y2h_event_record(y2h_event e, y2h_stream s);
int         y2h_event_sync(y2h_event e);                                        /* wait for the event only */
int         y2h_stream_wait_event(y2h_stream s, y2h_event e);                    /* later work on s runs after e (device-side wait) */
int         y2h_event_elapsed_ms(y2h_event start, y2h_event stop, float *ms);   /* syncs on stop */

/* ---- hipGraph capture of a kernel sequence on a stream (replaces nothing in the reference: its GPU path launches
 * every kernel from the host each call) ---- */
int  y2h_graph_begin(y2h_stream s);                   /* start recording what is enqueued on s (nothing executes) */
int  y2h_graph_end(y2h_stream s, y2h_graph *out);      /* stop recording, instantiate */
void y2h_graph_abort(y2h_stream s);                   /* leave capture mode after an error, keep nothing */
int  y2h_graph_launch(y2h_graph g, y2h_stream s);
int  y2h_graph_destroy(y2h_graph g);

/* ---- layout ---- */
/* [n][c][h][w] -> [n][h][w][ld] (channels 0..c-1 of each pixel row) and back; a NULL pointer or ld < c: Y2H_EINVAL */
int y2h_nchw_to_nhwc(const float *src, float *dst, int n, int c, int h, int w, int ld, y2h_stream s);
int y2h_nhwc_to_nchw(const float *src, int ld, float *dst, int n, int c, int h, int w, y2h_stream s);
/* [n][c][h][w] -> interior of [n][h+2*halo][w+2*halo][ld]; the border is not written
 * (the caller zeroes the buffer once); a NULL pointer, ld < c or halo < 0: Y2H_EINVAL */
int y2h_nchw_to_nhwc_halo(const float *src, float *dst, int n, int c, int h, int w, int ld, int halo, y2h_stream s);
/* copy `c` channels of `npix` pixels between two NHWC buffers ([route] fallback) */
int y2h_copy_channels(const float *src, int ld_src, float *dst, int ld_dst, int c, long npix, y2h_stream s);

/* ---- convolution + fused epilogue ---- */
typedef struct y2h_conv {
    int batch, h, w, c;          /* input  NHWC dims                                   */
    int ldx;                     /* input  channel stride (floats)                     */
    int x_halo;                  /* 0, or p > 0: x is [batch][h+2p][w+2p][ldx] with a zero border of p pixels
                                    (layout of y2h_nchw_to_nhwc_halo; first-layer / stem kernels only) */
    int n;                       /* filters (output channels)                          */
    int size, stride, pad;       /* square kernel                                      */
    int out_h, out_w;
    int ldy;                     /* output channel stride (floats)                     */
    int fuse_maxpool2;           /* 1: a 2x2 stride-2 pad-0 maxpool follows the activation inside
                                    the kernel; y is then [batch][out_h/2][out_w/2][ldy]
                                    (matrix-core kernels only, out_h and out_w even)   */
    int batch_normalize;         /* 1: (x-mean)*rinv*scale + bias ; 0: x + bias        */
    int activation;              /* Y2H_ACT_*                                          */
    const float  *x;             /* device, NHWC                                       */
    const float  *w_packed;      /* device, [n][size][size][c]                         */
    const float  *w_ref;         /* device, [n][c][size][size] (strict path only) or 0 */
    const float  *mean;          /* device [n]  rolling_mean        (BN only)          */
    const double *rinv;          /* device [n]  1/(sqrt((double)var)+1e-6f) (BN only)  */
    const float  *scale;         /* device [n]  scales              (BN only)          */
    const float  *bias;          /* device [n]                                         */
    float        *y;             /* device, NHWC (already offset to the first channel) */
    float        *ws;            /* device scratch for split-K partial sums, or 0      */
    size_t        ws_bytes;      /* size of ws; see y2h_conv_workspace_bytes           */
    /* fp16 storage (engine extension, the reference is fp32 only): */
    int           x_f16;         /* 1: x and w_packed hold IEEE half (ldx counts halves); fp32 accumulate on
                                    v_mfma_f32_32x32x16_f16; the epilogue is y = act(acc*alpha + beta)   */
    int           y_f16;         /* 1: y is stored as half (ldy counts halves)         */
    const float  *alpha;         /* device [n]  scale/(sqrt(var)+1e-6)  (1 without BN)  */
    const float  *beta;          /* device [n]  bias - mean*alpha                       */
    /* tile choice of the matrix-core kernel: 0 = the host's cost model decides (see y2h_conv_candidates) */
    int           tile_bm, tile_bn;   /* GEMM tile (output pixels x filters), one of the instantiated shapes */
    int           ksplit;             /* K ranges per output tile (1 = no split-K) */
    /* first layer only: x is the network input itself, fp32 planes [batch][c][h][w] (no NHWC copy) */
    int           x_nchw;
} y2h_conv;

/* Measure instead of model: the (tile_bm, tile_bn, ksplit) combinations worth timing for this descriptor, for callers
 * that measure in their own context (the engine, y2_set_autotune, times them inside whole forward passes, where the
 * caches hold what they hold in production); entry 0 is the cost model's choice.  Every tile shape accumulates each
 * output in the same K order, so the choice of tile never changes a result bit; a K-split does (partial sums are added
 * in a fixed order).  Returns the count (0: not an fp32 matrix-core convolution). */
int y2h_conv_candidates(const y2h_conv *d, int *bm, int *bn, int *ks, int max);

/* 1 if a first-layer kernel can read the fp32 NCHW network input directly (x_nchw = 1; 3 channels, 3x3/1 pad 1,
 * <= 64 filters; y_f16 as in the descriptor): no input transform kernel at all */
int y2h_conv_first_layer_nchw_ok(const y2h_conv *d);

/* which kernel y2h_conv_forward would pick: 1 = MFMA implicit GEMM, 0 = direct VALU */
int y2h_conv_uses_mfma(const y2h_conv *d);
/* bytes of split-K scratch y2h_conv_forward needs for this descriptor (0 = none): small grids
 * (13x13 maps at small batch, batch-1 inference) are cut along K so that all 256 CUs get work */
size_t y2h_conv_workspace_bytes(const y2h_conv *d);
/* Stream-K plan of the fp16 256x256 persistent kernel (replaces nothing in the reference: its GEMM is one cuBLAS call per
 * image, convolutional_kernels.cu:108-116): of `ntiles` output tiles of `nk` K-tiles each on a persistent grid of `grid`
 * workgroups, the last *sk_tiles are cut along K into equal shares for workgroups 0 .. *sk_wgs - 1 and finished by a
 * fix-up launch.  Returns 1 when the plan splits, 0 when every tile is walked whole.  Host arithmetic only (no GPU). */
int y2h_p8_stream_k_plan(long ntiles, int nk, long grid, int *sk_tiles, int *sk_wgs);
/* The stream-K share rule as every kernel compiles it (include/y2_streamk_rule.h: `tiles` tiles of nk K-steps dealt to G
 * workgroups), one call for all workgroups / tiles.  Host arithmetic only.  Each returns -1 unless 1 <= tiles <= G, nk >= 1.
 * y2h_sk_shares: out[5 w ..] = pieces (0, 1, 2), tile, kb0, ke0, ke1 of workgroup w.  y2h_sk_first: out[t] = the first share
 * that reaches into tile t.  y2h_sk_walk: the walk of every tile in turn, out[3 i ..] = tile, workgroup, piece (1: the share
 * began in the previous tile); returns the number of visits (at most tiles + G; -1 if `max` triples do not hold them). */
int y2h_sk_shares(long tiles, int nk, long G, int *out);
int y2h_sk_first(long tiles, int nk, long G, int *out);
int y2h_sk_walk(long tiles, int nk, long G, int *out, int max);
/* number of stream-K launches (main + fix-up pairs) issued by this process so far (tests, benchmark reports) */
unsigned long y2h_stream_k_launches(void);
/* number of small-tile tail launches behind the fp16 256x256 kernel (the other way to finish a partial last round) */
unsigned long y2h_tail_launches(void);
/* number of fp32 matrix-core launches that used the XCD-grouped tile order (wide heads: yolo9000's final 1x1) */
unsigned long y2h_xcd_order_launches(void);
/* number of fp32 matrix-core launches that used stream-K work items (grids smaller than the machine) */
unsigned long y2h_f32_stream_k_launches(void);
/* 1 when the shape fits the dedicated first-layer kernel (3 channels, 3x3/1 pad 1, <= 64
 * filters) provided the input is supplied with a halo (x_halo = 1) */
int y2h_conv_first_layer_ok(const y2h_conv *d);
/* halo width (>= 0) the few-channel stem kernel wants for this shape (any size / stride with pad as the halo, c <= 4,
 * <= 128 filters: the 7x7/2 stems of cfg/yolov1/yolo.cfg, resnet50.cfg, extraction.cfg), or -1 when the shape does
 * not fit it; pass the descriptor back with x_halo set to that value */
int y2h_conv_stem_halo(const y2h_conv *d);
/* same for the fp16 first-layer kernel, whose input is [batch][h+2][w+2][4] halves (x_f16 = 1, ldx = 4,
 * layout of y2h_nchw_to_nhwc4_halo_f16) and whose weights stay the fp32 packed [n][27] */
int y2h_conv_first_layer_f16_ok(const y2h_conv *d);
/* strict != 0 forces the direct kernel, which accumulates in the reference's exact
 * order (ci, kh, kw ascending; product and sum rounded separately: gemm.c:74-88)
 * and is therefore bit-identical to the CPU path; needs w_ref. */
int y2h_conv_forward(const y2h_conv *d, int strict, y2h_stream s);
/* name of the kernel variant last chosen for this descriptor (for profiles) */
const char *y2h_conv_variant(const y2h_conv *d, int strict);

/* ---- Winograd F(2x2,3x3) for the fp32 stride-1 3x3 convolutions (the rule: include/y2_wino_rule.h) ---- */
typedef struct y2h_wino {
    int eligible;                /* the shape is one the three Winograd kernels take                       */
    int take;                    /* the rule's answer (Y2_WINO=0: never, Y2_WINO=1: every eligible layer)   */
    int bm, bn;                  /* tile of the batched GEMM                                               */
    long tiles, tiles_pad;       /* 2x2 output patches per component, and padded to a multiple of bm       */
    size_t u_bytes;              /* transformed filters U[16][n][c]                                        */
    size_t v_bytes, m_bytes;     /* transformed input V[16][tiles_pad][c] and raw products M[16][tiles_pad][n] */
    double direct_cost, gemm_cost, wino_cost;   /* CU cycles, as the tile cost model counts them           */
} y2h_wino;
/* Host arithmetic only (no GPU).  Leaves what y2h_conv_variant / _candidates / _workspace_bytes / _uses_mfma answer alone. */
int y2h_wino_plan(const y2h_conv *d, y2h_wino *out);
/* bytes of scratch (V and M) y2h_conv_wino_forward needs in d->ws when the rule takes the descriptor, else 0 */
size_t y2h_wino_workspace_bytes(const y2h_conv *d);
/* The convolution as input transform -> batched GEMM -> output transform + epilogue.  d->w_packed holds U[16][n][c]
 * (y2_wino_filter of every (filter, channel), component-major), d->ws at least y2h_wino_workspace_bytes(d).  Y2H_EINVAL
 * unless y2h_wino_plan takes the descriptor. */
int y2h_conv_wino_forward(const y2h_conv *d, y2h_stream s);
/* number of such forwards issued by this process so far (tests) */
unsigned long y2h_wino_launches(void);

/* ---- the split form of the Winograd GEMM: fp32 operands as three bf16 planes (the rule: include/y2_split_rule.h) ---- */
typedef struct y2h_wino_split {
    int eligible;                /* the shape is one the split kernels take                                      */
    int take;                    /* the rule's answer (Y2_WINO_SPLIT=0: never, =1: every eligible layer)          */
    int bm, bn, bk;              /* tile of the batched GEMM                                                     */
    long tiles, tiles_pad;       /* 2x2 output patches per component, and padded to a multiple of bm             */
    size_t u_bytes;              /* split filters U[16][rows_pad(n)][c], three bf16 planes (y2_split_index)      */
    size_t v_bytes, m_bytes;     /* split input V[16][tiles_pad][c] (6 bytes per element), fp32 M[16][tiles_pad][n] */
    double present_cost, gemm_cost, split_cost;   /* CU cycles; present: the form the layer has without the split, fp32
                                                     Winograd or direct (zero when a switch decides, not the rule) */
} y2h_wino_split;
/* Host arithmetic only (no GPU).  Leaves what y2h_wino_plan, y2h_winos_plan and the conv queries answer alone. */
int y2h_wino_split_plan(const y2h_conv *d, y2h_wino_split *out);
/* bytes of scratch (V at 6 bytes per element, and M) y2h_conv_winox_forward needs in d->ws when the rule takes the descriptor, else 0 */
size_t y2h_wino_split_workspace_bytes(const y2h_conv *d);
/* The convolution as split input transform -> split GEMM -> output transform + epilogue.  d->w_packed holds the split U
 * (y2_split_pack_u), d->ws at least y2h_wino_split_workspace_bytes(d).  Y2H_EINVAL unless y2h_wino_split_plan takes the descriptor. */
int y2h_conv_winox_forward(const y2h_conv *d, y2h_stream s);
/* number of split GEMM launches issued by this process so far (tests) */
unsigned long y2h_wino_split_launches(void);

/* ---- stationary Winograd: F(2x2,3x3) as one fused kernel, filters in registers (the rule: include/y2_winos_rule.h) ---- */
typedef struct y2h_winos {
    int eligible;                /* the shape is one a form of the kernel takes                              */
    int take;                    /* the rule's answer (Y2_WINOS=0: never, Y2_WINOS=1: every eligible layer)  */
    int form;                    /* input channels of the form that takes it (32), 0: none                   */
    long patches;                /* 8 x 16-pixel output patches the persistent grid walks                    */
    size_t u_bytes;              /* transformed filters in the kernel's register order (y2_winos_u_index)    */
} y2h_winos;
/* Host arithmetic only (no GPU).  Leaves what every other query answers alone; needs no workspace. */
int y2h_winos_plan(const y2h_conv *d, y2h_winos *out);
/* The convolution as one launch.  d->w_packed holds U in register order (y2_winos_u_index of y2_wino_filter of every
 * (filter, channel)).  Y2H_EINVAL unless y2h_winos_plan takes the descriptor. */
int y2h_conv_winos_forward(const y2h_conv *d, y2h_stream s);
/* number of such forwards issued by this process so far (tests) */
unsigned long y2h_winos_launches(void);

/* ---- direct 3x3 convolution on the bf16 matrix cores by 3-way split (the rule: include/y2_splitd_rule.h) ---- */
typedef struct y2h_splitd {
    int eligible;                /* the shape is one the kernel takes and the direct plan is the fp32 matrix-core kernel */
    int take;                    /* the rule's answer (Y2_SPLITD=0: never, Y2_SPLITD=1: every eligible layer)             */
    int bm, bn, bk;              /* tile: positions x filters, K-tile                                                    */
    long tiles;                  /* tiles the persistent grid walks (position tiles x filter tiles)                      */
    size_t u_bytes;              /* split filters, three bf16 planes (y2_splitd_u_index)                                 */
    size_t lds_bytes;            /* LDS of the launch                                                                    */
    double direct_cost, matrix_cost, byte_cost, splitd_cost;   /* CU cycles; the larger of matrix and byte is the cost   */
} y2h_splitd;
/* Host arithmetic only (no GPU).  Leaves what every other query answers alone; needs no workspace. */
int y2h_conv_splitd_plan(const y2h_conv *d, y2h_splitd *out);
/* The convolution as one launch.  d->w_packed holds the split filters (y2_splitd_pack_u with y2_splitd_bn(n, pool)).  Y2H_EINVAL
 * unless y2h_conv_splitd_plan takes the descriptor. */
int y2h_conv_splitd_forward(const y2h_conv *d, y2h_stream s);
/* number of such forwards issued by this process so far (tests) */
unsigned long y2h_conv_splitd_launches(void);

/* ---- other layers (NHWC) ---- */
int y2h_maxpool(const float *x, int ldx, float *y, int ldy, int batch, int h, int w, int c,
                int size, int stride, int pad, int out_h, int out_w, y2h_stream s);
/* the reference's reorg quirk (blas.c:8-29 called with forward=0 for a non-reverse
 * layer, reorg_layer.c:83), re-expressed for NHWC in and out; reverse!=0 is forward=1 */
int y2h_reorg(const float *x, int ldx, float *y, int ldy, int batch, int h, int w, int c,
              int stride, int reverse, y2h_stream s);
/* [connected] in the reference's accumulation order (connected_layer.c:141-176 / gemm.c:90-106 gemm_nt): input element
 * k = c*hw + p of batch item b is x[b*x_batch_stride + p*ld + c] (an NHWC producer; hw = 1 for a flat one), weights
 * w_ref [outputs][hw*c] in the reference layout; BN / bias / activation as for a convolution */
int y2h_connected_ref(const float *x, long x_batch_stride, int ld, int hw, int c, const float *w_ref, float *y,
                      int outputs, int batch, int batch_normalize, int activation, const float *mean,
                      const double *rinv, const float *scale, const float *bias, y2h_stream s);
/* YOLOv1 head decode (detection_layer.c:222-251): pred = [batch] blocks of pred_stride floats; boxes
 * [batch][side*side*num][4], probs [batch][side*side*num][classes] */
int y2h_detection_boxes(const float *pred, long pred_stride, int batch, int side, int num, int classes, int sqrt_flag,
                        int w, int h, float thresh, int only_objectness, float *boxes, float *probs, y2h_stream s);
/* residual add (shortcut_layer.c:38-43, blas.c:57-81): out = act(in + add) where the shapes overlap; `add` is
 * w1 x h1 x c1, in/out are w2 x h2 x c2; stride = w1/w2 and sample = w2/w1 (each >= 1) as in shortcut_cpu.
 * activation: Y2H_ACT_LINEAR .. _RELU, the four evaluated inside the kernel (any other code: Y2H_EINVAL -- the engine passes
 * y2_act_for_kernel() and runs y2h_activate_array behind); w1/w2 != h1/h2 or w2/w1 != h2/h1 (blas.c:61-62): Y2H_EINVAL */
int y2h_shortcut(const float *in, int ld_in, const float *add, int ld_add, float *out, int ld_out, int batch,
                 int w1, int h1, int c1, int w2, int h2, int c2, int activation, y2h_stream s);
/* [crop] at inference (crop_layer.c:69-105, !state.train): centred out_h x out_w window, x*2-1 unless noadjust.
 * halo > 0: y is [batch][out_h+2*halo][out_w+2*halo][ldy] and only its interior is written (the caller zeroes it once) */
int y2h_crop(const float *x, int ldx, float *y, int ldy, int batch, int h, int w, int c, int out_h, int out_w,
             int noadjust, int halo, y2h_stream s);
/* standalone [batchnorm] at inference (batchnorm_layer.c:122-146): ((x - mean) * rinv) * scale per channel, rinv =
 * 1 / (sqrt(var) + 1e-6f) prepared in double (blas.c:122) */
int y2h_batchnorm(const float *x, int ldx, float *y, int ldy, long pixels, int c, const float *mean, const double *rinv,
                  const float *scale, y2h_stream s);
/* [local] (local_layer.c:95-126): per-location filter banks.  w_packed [location][filter][kh][kw][c], bias_packed
 * [location][filter] (the engine re-orders the reference's [location][filter][c][kh][kw] / [filter][location]);
 * strict = 1 runs the reference's summation order (bias first, taps in c,kh,kw order, one rounding per step).
 * activation: Y2H_ACT_LINEAR .. _RELU in both forms, any other code: Y2H_EINVAL (as y2h_shortcut); a last window that leaves
 * the padded image, (out_h - 1) * stride + size - pad > h + pad (or the same in w): Y2H_EINVAL */
int y2h_local(const float *x, int ldx, const float *w_packed, const float *bias_packed, float *y, int ldy, int batch,
              int h, int w, int c, int n, int size, int stride, int pad, int out_h, int out_w, int activation,
              int strict, y2h_stream s);
/* binarize_cpu (convolutional_layer.c:52-58) for xnor=1 convolutions: y[row][k] = x[row*ldx + k] > 0 ? 1 : -1, y contiguous */
int y2h_binarize(const float *x, int ldx, float *y, long rows, int c, y2h_stream s);
/* activate_array (activations.c:95-101, the formulas of activations.h:21-54) in place on channels 0..c-1 of `rows`
 * pixels with channel stride ld; any Y2H_ACT_* code */
int y2h_activate_array(float *x, int ld, long rows, int c, int activation, y2h_stream s);
/* [activation] (activation_layer.c:39-43): y[row*ldy + k] = act(x[row*ldx + k]) out of place, the same formulas in strict
 * and default mode, as y2h_activate_array.  _f16: half in and out, the function in fp32, Y2H_ACT_LINEAR .. _RELU only */
int y2h_activate_copy(const float *x, int ldx, float *y, int ldy, long rows, int c, int activation, y2h_stream s);
int y2h_activate_copy_f16(const void *x, int ldx, void *y, int ldy, long rows, int c, int activation, y2h_stream s);
/* [normalization] (normalization_layer.c:65-94), cross-channel LRN on NHWC: y = norm^-beta * x with
 * norm[k] = kappa + alpha * (sum of x[j]^2 over j in [k-(size-1)/2, k+size/2] within [0,c) - x[size/2]^2) -- the reference
 * never adds channel size/2 but subtracts it once it leaves the window.  Needs c >= max(1, size/2), size >= 1, ldx, ldy >= c.
 * strict = 0: one pass, squares staged in LDS, each window summed in ascending channel order, norm^-beta in fp32;
 * strict = 1 (and any c, size for which y2h_lrn_fast_ok is 0: more than 1024 channels): one lane per pixel in the reference's channel order with
 * pow in double, bit-identical to it.  A norm <= 0 gives a non-finite value, as in the reference.
 * y2h_lrn_f16: the one-pass form with half in and out, fp32 arithmetic (ld in halves); Y2H_EINVAL without y2h_lrn_fast_ok */
int y2h_lrn_fast_ok(int c, int size);
int y2h_lrn(const float *x, int ldx, float *y, int ldy, long pixels, int c, int size, float alpha, float beta, float kappa,
            int strict, y2h_stream s);
int y2h_lrn_f16(const void *x, int ldx, void *y, int ldy, long pixels, int c, int size, float alpha, float beta, float kappa,
                y2h_stream s);
/* global average pool: [batch][h*w][ld] -> [batch][c] (sequential fp32 sum, avgpool_layer.c:40) */
int y2h_avgpool(const float *x, int ldx, float *y, int batch, int h, int w, int c, y2h_stream s);
/* rows of `n` floats: softmax with temperature (blas.c:205); in/out may alias.  One workgroup per row, the exponentials in
 * LDS up to n = 12288 (48 KB), in the output row beyond.  A NULL pointer, rows or n <= 0, temp == 0: Y2H_EINVAL */
int y2h_softmax_rows(const float *x, float *y, long rows, int n, float temp, y2h_stream s);
/* softmax_tree (softmax_layer.c:35-47): every row of `n` floats is `groups` sibling groups [goff[g], goff[g] + gsize[g]),
 * each softmaxed on its own with y2h_softmax_rows' arithmetic (double exp, fp32 sum in index order); group_of[n] names
 * every element's group (tree.group).  The tables are device pointers; in/out may alias.  One workgroup per row with the
 * row in LDS while n + groups floats fit 64 KB, a thread per (row, group) in global memory beyond.
 * rows, n or groups <= 0 or a NULL pointer: Y2H_EINVAL. */
int y2h_softmax_tree_rows(const float *x, float *y, long rows, int n, float temp, int groups, const int *group_size,
                          const int *group_offset, const int *group_of, y2h_stream s);
/* hierarchy_predictions (tree.c:37-51) in place on `nrows` rows of `n` floats, `ld` floats apart: p[j] *= p[parent[j]] for j
 * ascending, then p[j] = 0 where !leaf[j] (leaf == NULL: no such step).  levels > 0: order / level_off are the nodes sorted
 * by depth and the level offsets (every parent precedes its child) and the row is walked level by level; levels == 0: the
 * sequential walk, whatever the order of the nodes.  row_mask (one int per row, NULL = every row): rows whose entry is 0
 * are left as they are. */
int y2h_hierarchy_rows(float *rows, long ld, int nrows, int n, const int *parent, const int *order, const int *level_off,
                       int levels, const int *leaf, const int *row_mask, y2h_stream s);

/* ---- half-storage variants (engine extension: BASELINE configs[4]; void* = IEEE half, ld in halves) ---- */
int y2h_maxpool_f16(const void *x, int ldx, void *y, int ldy, int batch, int h, int w, int c,
                    int size, int stride, int pad, int out_h, int out_w, y2h_stream s);
int y2h_reorg_f16(const void *x, int ldx, void *y, int ldy, int batch, int h, int w, int c,
                  int stride, int reverse, y2h_stream s);
int y2h_copy_channels_f16(const void *src, int ld_src, void *dst, int ld_dst, int c, long npix, y2h_stream s);
int y2h_avgpool_f16(const void *x, int ldx, float *y, int batch, int h, int w, int c, y2h_stream s);  /* fp32 sum and result */
int y2h_nhwc_f16_to_nchw(const void *src, int ld, float *dst, int n, int c, int h, int w, y2h_stream s);
/* fp32 [n][3][h][w] -> interior of half [n][h+2][w+2][4] (channel 3 = 0; the border is not written) */
int y2h_nchw_to_nhwc4_halo_f16(const float *src, void *dst, int n, int c, int h, int w, y2h_stream s);
int y2h_f32_to_f16(const float *src, void *dst, long n, y2h_stream s);
int y2h_f16_to_f32(const void *src, float *dst, long n, y2h_stream s);

/* ---- dense heads in fp16 storage mode ---- */
/* The K ranges of y2h_connected_f16 for `rows` x `inputs` x `outputs` (host arithmetic only, no GPU): *ranges K ranges,
 * each a whole number of 32-steps except the last, which ends at `inputs`; range r is [bounds[r], bounds[r + 1]) (bounds:
 * room for max_bounds ints, or NULL).  forced > 0 sets the count, clamped to the number of 32-steps; forced <= 0 lets the
 * cost model choose.  *ws_bytes = ranges * 16 * roundup(outputs, 16) * sizeof(float) of raw partial sums
 * ([range][16 rows][roundup(outputs, 16)]), 0 with one range. */
int y2h_connected_f16_plan(int rows, int inputs, int outputs, int forced, int *ranges, size_t *ws_bytes, int *bounds,
                           int max_bounds);
/* y[r][n] = act((sum_k x[r][k] * w[n][k]) * alpha[n] + beta[n]): x half [rows][ldx], w half [outputs][inputs], y fp32 or
 * half (y_f16) [rows][ldy], fp32 accumulation on the fp16 matrix cores, Y2H_ACT_LINEAR .. _RELU.  ranges / ws / ws_bytes as
 * y2h_connected_f16_plan gives them; partial sums are added in ascending K order (no atomics).  More than 16 rows run in
 * passes of 16. */
int y2h_connected_f16(const void *x, long ldx, const void *w, const float *alpha, const float *beta, void *y, int ldy,
                      int y_f16, int rows, int inputs, int outputs, int activation, int ranges, float *ws, size_t ws_bytes,
                      y2h_stream s);
/* y2h_local with half weights (same [location][filter][kh][kw][c] order), half input and output, fp32 accumulation and
 * fp32 biases; Y2H_ACT_LINEAR .. _RELU, any other code: Y2H_EINVAL */
int y2h_local_f16(const void *x, int ldx, const void *w_packed, const float *bias_packed, void *y, int ldy, int batch,
                  int h, int w, int c, int n, int size, int stride, int pad, int out_h, int out_w, int activation,
                  y2h_stream s);
/* y2h_crop reading fp32 and writing half NHWC; y4 (or NULL; c <= 4): also the interior of half [batch][out_h+2][out_w+2][4],
 * the input form of the fp16 first-layer kernel (the caller zeroes it once) */
int y2h_crop_f16(const float *x, int ldx, void *y, int ldy, void *y4, int batch, int h, int w, int c, int out_h, int out_w,
                 int noadjust, y2h_stream s);

/* ---- region head ---- */
/* x: last conv output NHWC [batch][h*w][ldx] holding num*(coords+1+classes) channels.
 * y: [batch][h*w*num][coords+1+classes] (the reference's flattened layout).
 * logistic on objectness, softmax (softmax!=0) or per-group tree softmax
 * (group_size/group_offset device arrays, groups>0) on the class scores. */
int y2h_region_forward(const float *x, int ldx, float *y, int batch, int hw, int num, int classes, int coords,
                       int softmax, int groups, const int *group_size, const int *group_offset, y2h_stream s);
/* The same for a tree head (groups > 0), with two options.
 * best != 0: from the class row still in LDS, what get_region_boxes needs of it in detect mode (region_layer.c:351-367
 *   without a map; tree.c:37-44): best[0 .. boxes) = hierarchy probability of the deepest class above .5 (0: none),
 *   best[boxes .. 2 boxes) = that class as int.  Independent of the detection threshold; y is written exactly as without.
 *   parent / order / level_off / levels: the tree with its nodes listed by depth level (parents precede children);
 *   y2h_region_tree_best_ok: 1 when the row fits the LDS kernel (classes <= 16383: the row and one word in 64 KB).
 * flags & Y2H_REGION_FAST_EXP: the group softmax takes expf (single precision, ~1 ulp) where the reference rounds a double
 *   exp to float (blas.c softmax): outputs differ by ~1e-7 relative, sums run in the reference's order.  The double exps are
 *   what the layer costs (9418 per box in yolo9000).  Env Y2_REGION_EXP_DOUBLE=1 overrides the flag. */
#define Y2H_REGION_FAST_EXP 1
int y2h_region_tree_best_ok(int classes, int levels);
int y2h_region_forward_tree(const float *x, int ldx, float *y, int batch, int hw, int num, int classes, int coords,
                            int groups, const int *group_size, const int *group_offset, const int *parent,
                            const int *order, const int *level_off, int levels, float *best, int flags, y2h_stream s);

typedef struct y2h_decode {
    int batch, w, h, num, classes;
    int img_w, img_h;               /* the (w,h) scale arguments of get_region_boxes   */
    float thresh;
    int only_objectness;
    int classfix;
    const float *anchors;           /* device [2*num]  (l.biases)                      */
    const int   *tree_parent;       /* device [classes] or 0 (softmax_tree)            */
    const int   *tree_order;        /* device [classes]: node ids sorted by depth, or 0; with
                                       tree_level_off [levels+1] and tree_levels > 0 the tree is
                                       walked level by level (valid only when every parent index
                                       is smaller than its children's: the caller checks)       */
    const int   *tree_level_off;
    int          tree_levels;
    const int   *map;               /* device [200] or 0                               */
    float       *pred;              /* device region output [batch][w*h*num][5+classes];
                                       the tree branch updates it in place, as the
                                       reference does (region_layer.c:350)            */
    float       *boxes;             /* device out [batch][w*h*num][4]                  */
    float       *probs;             /* device out [batch][w*h*num][classes]            */
} y2h_decode;
int y2h_region_boxes(const y2h_decode *d, y2h_stream s);

/* per-class sort + greedy suppression on device arrays, box.c:249-277.
 * probs rows have `stride` floats; only the first `classes` columns take part.
 * `probs_in` holds the scores and is only read (the tie order of the reference's
 * repeated stable sort depends on the original scores of earlier classes);
 * `probs` must be a separate copy of it, in which suppressed scores are zeroed.
 * `class_counts` is device scratch of batch*classes ints (non-zero scores per image and class: empty
 * classes are skipped). */
int y2h_nms_sort(const float *boxes, const float *probs_in, float *probs, int batch, int total, int classes,
                 int stride, float thresh, int *class_counts, y2h_stream s);
/* The chain get_region_boxes -> do_nms_sort -> compaction of a plain region head (no tree, no map, <= 256 classes) in three
 * (four for more than a million scores) launches: y2h_region_boxes + y2h_nms_sort (nms > 0) + y2h_collect with the same results (region_layer.c:328-379,
 * box.c:249-277, yolo_v2_class.cpp:221-238).  q->thresh is both the decode and the collect threshold.  `probs_nms` is the
 * copy the NMS suppresses in (the final scores when nms > 0; q->probs keeps the unsuppressed ones), `class_counts` is
 * batch * classes ints that must be zero on entry and are zero again on return.  y2h_detect_chain_ok: 1 if `q` qualifies. */
int y2h_detect_chain_ok(const y2h_decode *q);
int y2h_detect_chain(const y2h_decode *q, float nms, float *probs_nms, int *class_counts, float *records, int *counts,
                     int max_per_image, float *best_scratch /* 2 * batch * w*h*num floats, as y2h_collect, or 0 */, y2h_stream s);
/* The same chain for a TREE head without a class map (yolo9000 in detect mode) in two launches.  region_layer.c:351-367
 * leaves at most one non-zero score per box (the deepest class above .5, kept when the objectness exceeds q->thresh), so
 * the dense [boxes][classes] arrays of y2h_region_boxes / y2h_nms_sort / y2h_collect (261 MB per batch of yolo9000 544 b8,
 * walked six times) shrink to one (class, score) pair per box: same records and counts, no dense scores, and the prediction
 * rows are NOT edited in place.  Needs the level-ordered tree (tree_order / tree_level_off), q->thresh >= 0, no
 * only_objectness, <= 4096 boxes per image.  best_scratch: 2 * batch * w*h*num floats.  With `tree_best` (the region layer's
 * own by-product for these predictions) the class rows are not read again at all: three small launches. */
int y2h_detect_tree_chain_ok(const y2h_decode *q);
int y2h_detect_tree_chain(const y2h_decode *q, float nms, float *records, int *counts, int max_per_image, float *best_scratch,
                          const float *tree_best /* y2h_region_forward_tree's `best` for q->pred, or 0 */, y2h_stream s);
/* class-agnostic variant, box.c:279-298; total <= 16384 (one flag byte per box in LDS), Y2H_EINVAL beyond */
int y2h_nms(const float *boxes, float *probs, int batch, int total, int classes, int stride,
            float thresh, y2h_stream s);

/* compact detections per image in ascending box order (yolo_v2_class.cpp:221-238,
 * image.c:662-738): record = {x,y,w,h,prob,class} (6 floats); counts[b] = number found
 * (may exceed max_per_image; only the first max_per_image are stored). */
int y2h_collect(const float *boxes, const float *probs, int batch, int total, int classes, int stride,
                float thresh, float *records, int *counts, int max_per_image,
                float *best_scratch /* device, 2*batch*total floats */, y2h_stream s);

/* avg[i] = (0 + f[0][i] + f[1][i] + ... ) / n over n frames of `els` floats laid out back to back, summed in frame
 * order like utils.c:420-432 mean_arrays */
int y2h_mean_frames(const float *frames, int n, long els, float *avg, y2h_stream s);

/* separable align-corners bilinear resize of a CHW image (image.c:1950-1992) */
int y2h_resize_chw(const float *src, int c, int ih, int iw, float *tmp, float *dst, int h, int w, y2h_stream s);

/* ---- frame ingest: the steps in front of network_predict, on the device ---- */
/* `batch` 8-bit interleaved frames (h x w x c, row pitch `step` bytes, `frame_bytes` between frames) ->
 * float planes: dst[b][k][y][x] = (float)(src[..][k'] / 255.), k' = k with planes 0 and 2 exchanged when
 * swap_rb (BGR->RGB); only the first `planes` planes are written (a BGRA frame's alpha can be dropped).
 * yolo_v2_class.hpp:94-113,133-141; image.c:2045-2067,1181 */
int y2h_u8_to_planes(const unsigned char *src, int batch, int h, int w, int c, long step, long frame_bytes,
                     int planes, int swap_rb, float *dst, y2h_stream s);
int y2h_fill(float *dst, long n, float v, y2h_stream s);                                   /* image.c:1601 */
int y2h_embed_chw(const float *src, int c, int sh, int sw, float *dst, int dh, int dw, int dx, int dy,
                  y2h_stream s);                                                            /* image.c:1087 */
void y2h_letterbox_dims(int iw, int ih, int w, int h, int *new_w, int *new_h);             /* image.c:1607-1618 */
/* letterbox_image (image.c:1624): tmp holds c*ih*new_w + c*new_h*new_w floats */
int y2h_letterbox_chw(const float *src, int c, int ih, int iw, float *tmp, float *dst, int h, int w, y2h_stream s);

/* One item of y2h_regions_to_input: an ih x iw rectangle of 8-bit interleaved pixels that becomes batch slot b of the
 * network input.  Without a letterbox (nw, nh) is the network's size and dx = dy = 0; with one, (nw, nh) is
 * y2h_letterbox_dims of the region and (dx, dy) = ((w - nw) / 2, (h - nh) / 2).  The scales are computed on the host
 * exactly as y2h_resize_chw computes them: (float)(iw - 1) / (nw - 1) and (float)(ih - 1) / (nh - 1). */
typedef struct y2h_region {
    long long src;              /* byte offset of the item's first pixel from `pixels` */
    int pitch;                  /* bytes between rows */
    int c;                      /* bytes per pixel (channels) */
    int iw, ih;                 /* region size */
    int nw, nh;                 /* size it is resized to */
    int dx, dy;                 /* where that box sits in the network input */
    float w_scale, h_scale;
} y2h_region;

/* Fill the NCHW fp32 network input dst[batch][planes][h][w] in one launch from `n` regions (table `desc` of n
 * entries, in device memory, pointing into `pixels`).  Slot b < n equals, bit for bit, y2h_u8_to_planes of the region
 * followed by y2h_resize_chw to (nh, nw) -- or y2h_letterbox_chw: .5 outside the embedded box -- fused: every value is
 * formed by the same fp32 expressions in the same order.  Slots n .. batch-1 are set to 0. */
int y2h_regions_to_input(const y2h_region *desc, int n, const unsigned char *pixels, int batch, int planes, int swap_rb,
                         int h, int w, float *dst, y2h_stream s);

/* One item of y2h_regions_to_input_filtered: a y2h_region plus where its first pixel sits in the frame the aligned
 * depth8 plane belongs to, and the hand-crop distance filter of KinectUtil_with_cam.cpp:1866-1888.  filter == 0: the
 * item is read exactly as y2h_regions_to_input reads it. */
typedef struct y2h_region_f {
    y2h_region r;
    int fx, fy;                 /* frame position of the region's pixel (0, 0) */
    int filter;                 /* 1: a source pixel reads as 255 in every plane where y2_depth_whitens(depth8, far_limit) */
    float far_limit;            /* y2_far_limit(far_m), computed on the host in fp32 */
} y2h_region_f;

/* y2h_regions_to_input with that filter on the source read; depth8 is the H x W plane of y2h_depth_align (may be NULL
 * when no item filters), W its row length.  With every filter == 0 the result is bit-identical to y2h_regions_to_input. */
int y2h_regions_to_input_filtered(const y2h_region_f *desc, int n, const unsigned char *pixels, const unsigned char *depth8,
                                  int W, int batch, int planes, int swap_rb, int h, int w, float *dst, y2h_stream s);
/* The same with the grasp filter on top: where grasp16 (the H x W plane of y2h_plane_register, rows of W) is not NULL, a
 * filtered item also reads a source pixel as 255 in every plane when grasp16 is 0 under it.  grasp16 == NULL is
 * y2h_regions_to_input_filtered. */
int y2h_regions_to_input_grasp(const y2h_region_f *desc, int n, const unsigned char *pixels, const unsigned char *depth8,
                               const unsigned short *grasp16, int W, int batch, int planes, int swap_rb, int h, int w,
                               float *dst, y2h_stream s);

/* One item of y2h_augment_to_input: one image of load_data_detection (data.c:676-711).  `src` is a rectangle of the
 * 8-bit interleaved frame, rw x rh pixels whose first pixel is the frame's (x0, y0); it must hold every pixel the window
 * touches after constrain_int, i.e. columns clamp(pleft .. pleft + swidth - 1, 0, ow - 1) and the rows likewise (the kernel
 * clamps its taps into the rectangle, which never acts for such a descriptor).  The window may reach outside the frame
 * on every side.  The scales are computed on the host exactly as y2h_resize_chw computes them:
 * (float)(swidth - 1) / (w - 1) and (float)(sheight - 1) / (h - 1). */
typedef struct y2h_aug {
    long long src;              /* byte offset of the rectangle's first pixel from `pixels` */
    int pitch;                  /* bytes between its rows */
    int c;                      /* bytes per pixel (>= 3) */
    int x0, y0, rw, rh;         /* the rectangle inside the frame */
    int ow, oh;                 /* frame size */
    int pleft, ptop, swidth, sheight;       /* crop_image(orig, pleft, ptop, swidth, sheight) */
    int flip;
    float dhue, dsat, dexp;     /* distort_image(sized, dhue, dsat, dexp) */
    float w_scale, h_scale;
} y2h_aug;

/* Fill the dense NHWC fp32 training input dst[n][h][w][3] in one launch: per output pixel the (float)(v / 255.) plane
 * value, crop_image's constrain_int taps, resize_image's column and row pass, flip_image, rgb_to_hsv, the saturation and
 * exposure scales, the hue shift with its two wraps, hsv_to_rgb and constrain_image (image.c), every expression in the
 * reference's order and precision: bit for bit what that chain computes.  Channel k reads byte k of a pixel, 2 - k when
 * swap_rb.  No atomics, no reductions: the output is a pure function of the table. */
int y2h_augment_to_input(const y2h_aug *desc, int n, const unsigned char *pixels, int swap_rb, int h, int w, float *dst_nhwc,
                         y2h_stream s);

/* One item of y2h_augment_cls_to_input: one image of load_image_augment_paths (data.c:107-132).  `src` is a rectangle of
 * the 8-bit interleaved frame, rw x rh pixels whose first pixel is the frame's (x0, y0); it must hold every pixel a tap of
 * bilinear_interpolate touches after get_pixel_extend's clamp (y2_aug_cls_rect computes it; the kernel clamps into the
 * rectangle as well, which never acts for such a descriptor).  The crop may reach outside the frame on every side.
 * What does not depend on the output pixel is formed on the host, each the C expression's own operation chain:
 *   cosr, sinr   cos((double)rad), sin((double)rad) of the host's libm -- the device never computes them
 *   s, aspect    the floats, promoted
 *   ax, ay       dx / s * aspect and dy / s: float operations in C (all three operands are floats), then promoted
 *   cx, cy       (float)(ow / 2.), (float)(oh / 2.) */
typedef struct y2h_aug_cls {
    long long src;              /* byte offset of the rectangle's first pixel from `pixels` */
    double cosr, sinr, s, aspect, ax, ay;
    float cx, cy;
    int pitch;                  /* bytes between its rows */
    int c;                      /* bytes per pixel (>= 3) */
    int x0, y0, rw, rh;         /* the rectangle inside the frame */
    int ow, oh;                 /* frame size */
    int flip;
    float dhue, dsat, dexp;     /* distort_image(crop, dhue, dsat, dexp) */
} y2h_aug_cls;

/* Fill the dense NHWC fp32 training input dst[n][size][size][3] in one launch: per output pixel (x, y) -- column
 * size - 1 - x when flip, flip_image runs on the crop -- rotate_crop_image's rx and ry (image.c:1471-1472) in double,
 * operation for operation, rounded to float; bilinear_interpolate (image.c:1935-1948) with floorf, float weights and the
 * four get_pixel_extend taps of (float)(v / 255.) plane values summed left to right; then distort_image and
 * constrain_image exactly as y2h_augment_to_input does them.  Channel k reads byte k of a pixel, 2 - k when swap_rb.
 * No atomics, no reductions: the output is a pure function of the table. */
int y2h_augment_cls_to_input(const y2h_aug_cls *desc, int n, const unsigned char *pixels, int swap_rb, int size,
                             float *dst_nhwc, y2h_stream s);

/* ---- depth stage of the Kinect loop (y2_depth.hip; KinectUtil_with_cam.cpp:394-442, :1482-1706) ---- */
/* Register a dh x dw depth frame (and body-index frame, or NULL) to the H x W colour frame: for every colour pixel
 * (dx, dy) = y2_depth_coord of map[pixel] (NULL map: the pixel's own position, H == dh and W == dw); inside the depth
 * frame depth16 = depth, depth8 = depth >> 5, person = body (255 without one), dxy = (dx, dy); otherwise 0, 0, 255,
 * (-1, -1).  Streams 8 bytes of map in and 8 bytes of planes out per colour pixel. */
int y2h_depth_align(const unsigned short *depth, const unsigned char *body, const float *map, int dh, int dw, int H, int W,
                    unsigned short *depth16, unsigned char *depth8, unsigned char *person, short *dxy, y2h_stream s);

/* How the boxes of y2h_depth_boxes reach their frame: item b's boxes are mapped with these values by the expressions
 * of y2_region_box_to_frame in fp32 in the same order.  letterbox == 0 skips the first step, whole != 0 the second. */
typedef struct y2h_box_map {
    int letterbox, whole;
    int net_w, net_h, nw, nh;
    int rx, ry, rw, rh, fw, fh;
} y2h_box_map;

/* what y2h_depth_boxes writes per box: sr_yolo2.h y2_det3d, field for field */
typedef struct y2h_det3d {
    int valid, left, top, right, bot, otsu, mean_all_mm; float avg_mm; int body_id, belongs;
    float cam_x, cam_y, cam_z, cam_w, cam_h; float pts[5][2];
} y2h_det3d;

typedef struct y2h_depth_planes {
    const unsigned short *depth16; const unsigned char *depth8, *person;
    const short *dxy;           /* NULL: identity (the frame was registered already) */
    const float *cam_table;     /* dh x dw x 2, or NULL */
    int H, W, dh, dw;
    const unsigned short *grasp16;  /* NULL: the Demo_what statistics.  Otherwise the Grasp branch (:1508-1518): avg_mm =
                                       GetImgAvg(grasp16 ROI, 255 * 32) with no "- 16", otsu reported as 255 */
} y2h_depth_planes;

unsigned long y2h_depth_acc_bytes(void);     /* bytes of accumulator scratch per box */
/* Statistics of `items * per_item` box slots.  Slot (b, j) holds a box when j < min(counts[b], per_item) (counts == NULL:
 * every slot does); its box is the first four floats of boxes[(b * stride_item + j) * stride_box ...], mapped by maps[b]
 * (maps == NULL: used as it is).  The launch needs no count on the host: its size does not grow with the slots (up to 64
 * workgroups share a box, 128 rows of them walk the slots and skip the empty ones after one read of the count).  Results
 * are written DENSELY: item b's records follow item b-1's, out[sum_{i<b} min(counts[i], per_item) + j]; with counts ==
 * NULL that is out[b * per_item + j].  acc: items * per_item * y2h_depth_acc_bytes() of scratch.  `stages` selects what
 * is enqueued (Y2H_DEPTH_ALL for a result; single stages exist to be timed): clear the scratch, pass 1 over each ROI,
 * pass 2, finalise.  No synchronisation. */
enum { Y2H_DEPTH_CLEAR = 1, Y2H_DEPTH_PASS1 = 2, Y2H_DEPTH_PASS2 = 4, Y2H_DEPTH_FINALISE = 8, Y2H_DEPTH_ALL = 15 };
int y2h_depth_boxes(const y2h_depth_planes *p, const float *boxes, int stride_box, long stride_item, const int *counts,
                    const y2h_box_map *maps, int items, int per_item, void *acc, y2h_det3d *out, int stages, y2h_stream s);

/* ---- table-plane removal of the Grasp branch (y2_plane.hip; KinectUtil_with_cam.cpp:1931-1974, plane_seg.cpp:157-213;
 * the rule is include/y2_plane_rule.h) ---- */
/* the plane record: sr_yolo2.h y2_plane, field for field */
typedef struct y2h_plane { int found, best, valid_points, best_count, removed, pad_; double a, b, c, d; } y2h_plane;
#define Y2H_PLANE_COUNTS 260    /* ints of `counts`: one per hypothesis (256), the valid points at [256] */
typedef struct y2h_plane_job {
    const unsigned short *depth;    /* dh*dw, millimetres, as uploaded */
    const float *tab;               /* dh*dw*2, the camera table */
    const int *triples;             /* iters*3 depth-pixel indices; a void hypothesis is (-1, -1, -1) */
    long n;                         /* dh*dw */
    int iters;                      /* 1 .. 256 */
    float far_mm, dist_m;           /* y2_plane_far_mm(far_m); the inlier distance */
    int *counts;                    /* [Y2H_PLANE_COUNTS] */
    double *slab;                   /* [y2h_plane_chunks(n)][10]: one partial of the ten sums per chunk of the tree */
    y2h_plane *rec;
    unsigned short *grasp_depth;    /* dh*dw out: the clipped depth with the plane's pixels zeroed */
} y2h_plane_job;
unsigned long y2h_plane_chunks(long n);
/* Enqueue the stages selected (Y2H_PLANE_ALL for a result; single stages exist to be timed): clear the counts, count
 * every hypothesis' inliers, the refit sums of the best one, the fit and the record, the grasp depth.  No synchronisation,
 * no floating-point atomics: the result does not depend on the launch shape or on arrival order. */
enum { Y2H_PLANE_CLEAR = 1, Y2H_PLANE_COUNT = 2, Y2H_PLANE_SUMS = 4, Y2H_PLANE_FIT = 8, Y2H_PLANE_APPLY = 16, Y2H_PLANE_ALL = 31 };
int y2h_plane_remove(const y2h_plane_job *j, int stages, y2h_stream s);
/* grasp16[H][W] = grasp_depth under the (dx, dy) that y2h_depth_align wrote for the colour pixel, 0 where unmapped */
int y2h_plane_register(const unsigned short *grasp_depth, const short *dxy, int H, int W, int dw, unsigned short *grasp16,
                       y2h_stream s);

/* ---- KCF tracker of the Kinect loop (y2_kcf.hip; kcf.cpp, complexmat.hpp, piotr_fhog/) ---- */
#define Y2H_KCF_CHANNELS 31         /* fHOG channels kept of 32 */
#define Y2H_KCF_CHUNKS 32           /* partial sums of sqr_norm per tracker, added in chunk order */
#define Y2H_KCF_MAX_TRACKERS 32
#define Y2H_KCF_MAX_CELLS 256       /* feature map side; the window is 4x that in pixels */
/* One tracker: its window (pixels of the possibly halved image), its feature map (R = cells_h rows, C = cells_w columns,
 * P = R*C) and where its buffers start, as float offsets into the arena every kernel takes.  Complex tensors are two
 * planes, [re][R][C] then [im][R][C], per channel.
 *   patch win_h*win_w | mag, bin the same (bin holds ints) | hist 18*P | ssum P | feat 31*P | x 31*P (feat times the window)
 *   y, xf, model_xf 31*2*P | z, t, gy, kf, p, model_alphaf, yf 2*P | xy, g, resp, lab P | win R + C (row then column
 *   factors of the Hann window) | cc, nsc C*C: cos and -sin of 2*pi*((j*k) mod C)/C | cr, sr, nsr R*R: cos, sin, -sin of
 *   2*pi*((j*k) mod R)/R | part 2*Y2H_KCF_CHUNKS */
typedef struct y2h_kcf_desc {
    int resized, win_w, win_h, cells_w, cells_h, pad_;
    long long patch, mag, bin, hist, ssum, feat, x, y, xf, z, t, xy, g, gy, kf, p, resp, model_xf, model_alphaf, yf, lab, win,
              cc, nsc, cr, sr, nsr, part;
} y2h_kcf_desc;
/* what the arg-max leaves per tracker: the tracked centre in the tracker's own scale, the response maximum, its wrapped cell */
typedef struct y2h_kcf_rec { double cx, cy; float peak; int mx, my, pad_; } y2h_kcf_rec;
/* rows [row_lo, row_hi) of an h x w x c 8-bit frame (c = 1, 3: BGR, 4: BGRA), packed at w*c bytes per row */
typedef struct y2h_kcf_frame { const unsigned char *bytes; int h, w, c, row_lo, row_hi; } y2h_kcf_frame;
/* Every call serves the n trackers of the device table `desc` in one launch per kernel, on stream s, without
 * synchronisation.  max_pixels / max_cells / max_side: the largest win_w*win_h, cells_w*cells_h and cell side of the table
 * (they size the launch; a tracker's own sizes bound what is touched).
 * patch: grey ((1868*B + 9617*G + 4899*R + 8192) >> 14; one channel as is), for a resized tracker the half-resolution
 *   pixel formed on the fly (taps (-3, 19, 19, -3)/32 at 2d-1 .. 2d+2 clamped, horizontal then vertical, left to right),
 *   and get_subwindow (kcf.cpp:277-325) about (centres[t*stride], centres[t*stride + 1]) truncated to int. */
int y2h_kcf_patch(const y2h_kcf_desc *desc, int n, float *arena, const y2h_kcf_frame *f, const double *centres, int stride,
                  long max_pixels, y2h_stream s);
/* FHoG::extract(patch, 2, 4, 9) -> feat, and x = feat * window: gradient / orientation bin, the histogram gather, the
 * norm sums, the channels (four launches). */
int y2h_kcf_fhog(const y2h_kcf_desc *desc, int n, float *arena, long max_pixels, long max_cells, y2h_stream s);
/* Dense DFTs on the fp32 matrix cores, two launches each: x -> xf (31 channels), g -> kf, lab -> yf forward; z -> xy and
 * p -> resp inverse, real part only, scaled by 1/(R*C). */
enum { Y2H_KCF_DFT_X = 0, Y2H_KCF_DFT_G = 1, Y2H_KCF_DFT_LAB = 2, Y2H_KCF_IDFT_Z = 3, Y2H_KCF_IDFT_P = 4 };
int y2h_kcf_dft(const y2h_kcf_desc *desc, int n, float *arena, int which, int max_side, y2h_stream s);
/* z = sum over the channels of xf * conj(model_xf) (autocorrelation: |xf|^2) and the partial sums of both sqr_norms */
int y2h_kcf_cross(const y2h_kcf_desc *desc, int n, float *arena, int autocorrelation, y2h_stream s);
/* g = exp(-1/sigma^2 * max((xx + yy - 2*xy) / (P*31), 0)), sigma = 0.5 */
int y2h_kcf_gauss(const y2h_kcf_desc *desc, int n, float *arena, long max_cells, y2h_stream s);
/* alphaf = yf / (kf + 1e-4).  update == 0: model = (xf, alphaf).  Otherwise model = model * 0.98 + new * 0.02 and
 * pose[t] = (rec[t].cx, rec[t].cy). */
int y2h_kcf_train(const y2h_kcf_desc *desc, int n, float *arena, int update, double *pose, const y2h_kcf_rec *rec, long max_cells,
                  y2h_stream s);
/* p = model_alphaf * kf */
int y2h_kcf_apply(const y2h_kcf_desc *desc, int n, float *arena, long max_cells, y2h_stream s);
/* the first maximum of resp in row-major order, wrapped (> R/2, > C/2 with integer halves); rec = pose + 4 * cell */
int y2h_kcf_argmax(const y2h_kcf_desc *desc, int n, const float *arena, const double *pose, y2h_kcf_rec *rec, y2h_stream s);

/* ---- classifier views (classifier.c:336-593 valid10 / validmulti / validfull) ---- */
/* One view of y2h_views_to_input: a w x h window of a CHW fp32 source image that becomes batch slot b of the network
 * input.  The window's top-left corner sits at (dx, dy) of the source; both may be negative or reach past the source. */
typedef struct y2h_view {
    long long src;              /* float offset of the source image's first value from `src` */
    int sw, sh;                 /* source size; its planes lie sw*sh floats apart */
    int dx, dy;                 /* shift of the window */
    int flip;                   /* 1: the window is taken of the mirrored source (flip_image) */
    int pad_;
} y2h_view;

/* Fill the NCHW fp32 network input dst[batch][planes][h][w] in one launch from `n` views (table `desc` of n entries, in
 * device memory, pointing into `src`).  Slot b < n equals, bit for bit, crop_image(source, dx, dy, w, h)
 * (image.c:1512-1532), taken after flip_image (image.c:1056-1070) when flip is set:
 *     r = clamp(j + dy, 0, sh-1);  c = clamp(i + dx, 0, sw-1);  if (flip) c = sw-1-c;  dst[b][k][j][i] = source[k][r][c]
 * -- the reference's constrain_int: taps outside the source repeat its edge, they are not zero.  Slots n .. batch-1 are
 * set to 0.  Data movement only: 4 bytes read and 4 written per output value. */
int y2h_views_to_input(const y2h_view *desc, int n, const float *src, int batch, int planes, int h, int w, float *dst,
                       y2h_stream s);
/* acc[owner[s]][j] = acc[owner[s]][j] + rows[s][j] for the slots s = 0 .. nslots-1 in ascending order whose owner[s] >= 0
 * (`owner` in device memory; a negative owner's row is not read), j < n.  rows has row stride ld >= n, acc is
 * [..][n] contiguous.  One thread per column walks the slots in order: each sum is rounded once, in slot order, as
 * axpy_cpu(classes, 1, p, 1, pred, 1) adds one prediction after another (classifier.c:393,577,580).  Per accumulated row
 * 4 bytes read of `rows` and 4 read + 4 written of `acc` per value. */
int y2h_accumulate_rows(float *acc, const float *rows, int ld, const int *owner, int nslots, int n, y2h_stream s);

/* ---- recurrent layers ([rnn] / [gru], y2_recurrent.hip) ----
 * One launch computes n dense columns over `rows` (<= a few dozen) input rows, the sub-layer's epilogue (batch-norm with
 * the rolling statistics, bias, any activation, in the reference's order) and then the mode's combine:
 *   DENSE   out[r][j] = v                                          (a hoisted projection of a small batch)
 *   RNN     out[r][j] = ((shortcut ? state : 0) + proj[r][j]) + v  (rnn_layer.c:97-111); out2 (if set) gets a copy
 *   GRU_ZR  columns j < h:  out[r][j] = z = sigma(proj_z + v);  columns h + j:  out2[r][j] = f = state * sigma(proj_r + v)
 *   GRU_H   y = z*state + (1-z)*sigma(proj_h + v) -> out[r][j] (the state, in place: only column j reads it) and out2[r][j]
 * with proj = the step's rows of the hoisted input projections ([rows][h]; GRU: [rows][3h] = z | r | h columns) and
 * sigma(x) = (float)(1/(1+exp(-(double)x))) (gru_layer.c:154-171, blas.c:49-55).  Each product and sum is rounded on
 * its own.
 * form Y2H_REC_SKINNY: weight streaming -- the x rows are staged in LDS once per workgroup, a wave streams the weight
 * rows of its columns once with 16-byte loads, lanes split k and a fixed butterfly reduces (no atomics: two runs are
 * bitwise equal).  Needs y2h_rec_skinny_ok(rows, k).  Column j always runs in the same workgroup, so a step finds its
 * weight slice in the same XCD's L2 as the step before.
 * form Y2H_REC_REF: one thread per value, the dot product in the reference's order (gemm_nt, gemm.c:90-106), bit-identical
 * to the CPU path; with `pre` set the dense values are read from there instead (combine only). */
enum { Y2H_REC_DENSE = 0, Y2H_REC_RNN = 1, Y2H_REC_GRU_ZR = 2, Y2H_REC_GRU_H = 3 };
enum { Y2H_REC_REF = 0, Y2H_REC_SKINNY = 1 };
#define Y2H_REC_SKINNY_MAX_ROWS 8
typedef struct {
    const float *x;              /* [rows][k] input rows of the dense product                                */
    const float *w;              /* [n][k] weights (the reference's [outputs][inputs])                       */
    const float *bias, *mean, *scale;
    const double *rinv;          /* 1 / (sqrt(var) + 1e-6f) in double, as for a convolution                  */
    int bn, act;                 /* act: any Y2H_ACT_*                                                       */
    const float *pre;            /* [rows][n] dense values made elsewhere (Y2H_REC_REF only), or NULL        */
    int rows, k, n, h;
    int mode, shortcut;
    const float *proj;           /* hoisted input projections of this step                                  */
    const float *state;          /* [rows][h] state before the step                                          */
    float *out, *out2;
    const float *z;              /* GRU_H: [rows][h] z of this step                                          */
    float *xcopy;                /* if set, the launch also copies the x rows there ([rows][k])              */
} y2h_rec_args;
int y2h_rec_skinny_ok(int rows, int k);
int y2h_rec_step(const y2h_rec_args *a, int form, y2h_stream s);

/* ---- character generation and scoring on [rnn] / [gru] networks (y2_recurrent.hip) ----
 * y2h_rnn_sample: one workgroup per sequence b < seqs draws the next character from row b of `out` ([seqs][outputs], read
 *   only) by the rule of test_char_rnn (rnn.c:273-276) and sample_array (utils.c:520-531) over the first n values
 *   (n <= outputs, n <= 16384): a value < .0001 (compared in double) counts as 0; the fp32 sum ascending from 0; every
 *   value times (float)(1. / sum); r = u[b], r = r - a[i] ascending, the first i with r <= 0, else n - 1.  It writes
 *   next[b] = i and moves the 1 of input row b (x: [seqs][n]) from column prev[b] to column i.  probs (if set) receives
 *   the rows as they are, [seqs][outputs].
 * y2h_rnn_feed: x[r][j] = (tok[r] == j) for r < rows -- the one-hot input rows of one forward, step-major like tok.
 * y2h_rnn_score: p_next[r] = out[r][next[r]] for r < rows; probs (if set) receives the rows, [rows][outputs].
 * Tokens must lie in [0, inputs) / [0, outputs): the callers check them on the host. */
int y2h_rnn_sample(const float *out, int outputs, int n, int seqs, const float *u, const int *prev, int *next, float *x,
                   float *probs, y2h_stream s);
int y2h_rnn_feed(const int *tok, float *x, int rows, int inputs, y2h_stream s);
int y2h_rnn_score(const float *out, int outputs, const int *next, int rows, float *p_next, float *probs, y2h_stream s);
unsigned long y2h_rnn_sample_launches(void);     /* y2h_rnn_sample launches of this process */

/* ---- training (y2_train.hip): the reference's forward(train) / backward / update loop nests, fp32 ----
 * Activations and deltas are dense NHWC ([batch][h][w][c], no channel stride).  Trainer weights are [size][size][c][n]
 * (row (ky*size + kx)*c + ci, column filter): a pure permutation of the host's [n][c][size][size].
 * The three products of a stride-1 convolution run as one implicit-GEMM kernel on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 sums), 64x64 output tiles, operands gathered straight from the NHWC
 * tensors with guarded edges (any channel count, any image size, any size / pad):
 *   forward   y[m][f]   = sum_k  x(m, k) * w[k][f]            m = (b, oy, ox), k = (ky, kx, ci)
 *   dinput    dx[p][ci] = sum_r dy(p, r) * w[(ky, kx, ci)][f]  p = (b, iy, ix), r = (ky, kx, f)
 *   dweight   dw[k][f] += sum_m  x(m, k) * dy[m][f]            the reduction over m is cut into y2h_train_dweight_splits
 *             ranges, a function of the shape alone; every range writes its own partial tile into `ws`, and a second
 *             launch adds the partials to dw in range order.  No atomics: two runs give the same bytes.
 * Every other reduction (per-channel sums, the cost) uses a fixed split with a second pass or a fixed tree as well. */
typedef struct { int batch, h, w, c, n, size, pad, out_h, out_w; } y2h_train_conv;
int    y2h_train_conv_forward(const y2h_train_conv *g, const float *x, const float *w, float *y, y2h_stream s);
int    y2h_train_conv_dinput(const y2h_train_conv *g, const float *dy, const float *w, float *dx, y2h_stream s);
int    y2h_train_dweight_splits(const y2h_train_conv *g);
size_t y2h_train_dweight_ws_bytes(const y2h_train_conv *g);
int    y2h_train_conv_dweight(const y2h_train_conv *g, const float *x, const float *dy, float *dw, float *ws, y2h_stream s);
/* The same three products on the bf16 matrix cores (y2_train_bf16.hip), fp32 in and out, fp32 accumulation.  planes = 3: every
 * operand value is split into three bf16 numbers (include/y2_split_rule.h) and the six products of order <= 2 are summed,
 * smallest first -- fp32 results but for terms below 2^-25 |a b|.  planes = 1: every operand value is rounded once to bf16,
 * to nearest even.  Same shapes, same refusals, same workspace and the same reduction ranges and second pass for the weight
 * gradient as the fp32 entries; any other `planes` is Y2H_EINVAL. */
int    y2h_train_conv_forward_bf16(const y2h_train_conv *g, const float *x, const float *w, float *y, int planes, y2h_stream s);
int    y2h_train_conv_dinput_bf16(const y2h_train_conv *g, const float *dy, const float *w, float *dx, int planes, y2h_stream s);
int    y2h_train_conv_dweight_bf16(const y2h_train_conv *g, const float *x, const float *dy, float *dw, float *ws, int planes, y2h_stream s);
/* The three products of a dense ([connected]) layer (y2_train_dense.hip; connected_layer.c:122-190), fp32 in and out on the
 * fp32 matrix cores in EVERY training precision: y2_train_set_precision steers the convolutions' products only.
 * x is [batch][inputs], d and y [batch][outputs], w and dw [outputs][inputs]; any batch, inputs, outputs >= 1 (edges are
 * guarded, rows beyond 32 run as further passes).
 *   forward   y[b][o]   = sum_k x[b][k] * w[o][k]     K is cut into ranges of whole 32-steps so that the whole chip streams w once
 *   dinput    dx[b][k]  = sum_o d[b][o] * w[o][k]     (add != 0: +=); the outputs are cut into ranges of whole 64-steps
 *   dweight   dw[o][k] += sum_b d[b][o] * x[b][k]     a rank-batch update: every dw element is read and written once, no workspace
 * With more than one range every range writes raw partial sums to ws[range][batch][outputs | inputs] and a second launch
 * adds them in ascending range order: no atomics, two runs give the same bytes.  y2h_train_dense_plan (host arithmetic, no
 * GPU) gives the range count -- a function of the shape alone, unless forced > 0 or Y2_TRAIN_DENSE_KSPLIT=n sets it, clamped
 * to the steps of the layer (tests) --, the workspace bytes (0 with one range) and, in bounds[0 .. ranges], the ranges'
 * ends.  The entries take the same `forced`; ws may be NULL when the plan asks for no bytes. */
typedef struct { int batch, inputs, outputs; } y2h_train_dense;
enum { Y2H_DENSE_FORWARD = 0, Y2H_DENSE_DINPUT = 1 };
int y2h_train_dense_plan(const y2h_train_dense *g, int product, int forced, int *ranges, size_t *ws_bytes, int *bounds, int max_bounds);
int y2h_train_dense_forward(const y2h_train_dense *g, const float *x, const float *w, float *y, float *ws, int forced, y2h_stream s);
int y2h_train_dense_dinput(const y2h_train_dense *g, const float *d, const float *w, float *dx, int add, float *ws, int forced, y2h_stream s);
int y2h_train_dense_dweight(const y2h_train_dense *g, const float *x, const float *d, float *dw, y2h_stream s);
/* per-channel sums over rows = batch * spatial pixels; `scratch` holds y2h_train_reduce_scratch_bytes(rows, c) bytes.
 *   stats     batchnorm_layer.c:129-137: mean, variance (/(rows-1)), rolling = .9f * rolling + .1f * new  (two sweeps)
 *   bias      backward_bias (+ backward_scale_cpu when x_norm != NULL): bias_updates += sum delta, scale_updates += sum delta*x_norm
 *   bn_deltas scale_bias on delta, mean_delta_cpu and variance_delta_cpu in one sweep; delta itself is left unscaled:
 *             y2h_train_bn_backward multiplies by the scale again while it applies normalize_delta_cpu */
size_t y2h_train_reduce_scratch_bytes(long rows, int c);
int y2h_train_bn_stats(const float *x, long rows, int c, float *mean, float *variance, float *rolling_mean,
                       float *rolling_variance, float *scratch, y2h_stream s);
/* the same with the rolling statistics' two constants given: rolling = keep * rolling + take * new (a [connected] layer's
 * are .95f and .05f, connected_layer.c:138-141; y2h_train_bn_stats is keep = .9f, take = .1f) */
int y2h_train_bn_stats_rate(const float *x, long rows, int c, float *mean, float *variance, float *rolling_mean,
                            float *rolling_variance, float keep, float take, float *scratch, y2h_stream s);
int y2h_train_bias_grad(const float *delta, const float *x_norm, long rows, int c, float *bias_updates, float *scale_updates,
                        float *scratch, y2h_stream s);
int y2h_train_bn_deltas(const float *delta, const float *x, const float *scales, const float *mean, const float *variance,
                        long rows, int c, float *mean_delta, float *variance_delta, float *scratch, y2h_stream s);
int y2h_train_bn_backward(float *delta, const float *x, const float *scales, const float *mean, const float *variance,
                          const float *mean_delta, const float *variance_delta, long rows, int c, y2h_stream s);
/* y (the raw product, in place): with mean != NULL x = y, x_norm = (y - mean) / (sqrt(var) + 1e-6f), y = x_norm * scale;
 * then y = act(y + bias) (convolutional_layer.c:466-472) */
int y2h_train_bn_apply(float *y, float *x, float *x_norm, const float *mean, const float *variance, const float *scales,
                       const float *biases, int act, long rows, int c, y2h_stream s);
int y2h_train_act_gradient(const float *y, float *delta, int act, long n, y2h_stream s);   /* gradient_array */
/* maxpool_layer.c:79-117: the first maximum in (row, column) scan order, strict >, padding reads as -FLT_MAX; idx holds
 * iy * w + ix of the winner (-1: none).  Backward gathers, per input pixel, the windows that cover it in output order. */
int y2h_train_maxpool_forward(const float *x, float *y, int *idx, int batch, int h, int w, int c, int size, int stride, int pad,
                              int out_h, int out_w, y2h_stream s);
int y2h_train_maxpool_backward(const float *dy, const int *idx, float *dx, int batch, int h, int w, int c, int size, int stride,
                               int pad, int out_h, int out_w, y2h_stream s);
int y2h_train_avgpool_forward(const float *x, float *y, int batch, int hw, int c, y2h_stream s);
int y2h_train_avgpool_backward(const float *dy, float *dx, int batch, int hw, int c, y2h_stream s);
int y2h_train_softmax(const float *x, float *y, int rows, int n, float temperature, y2h_stream s);
/* l2_cpu + sum_array (cost_layer.c:85-87) and backward_cost_layer into a zeroed delta: delta = truth - pred,
 * error = delta^2 (the layer's output), cost[0] = sum error (fixed tree), delta_prev = scale * delta */
int y2h_train_cost_sse(const float *pred, const float *truth, float *error, float *delta, float *delta_prev, float scale, long n,
                       float *cost, y2h_stream s);
/* the same over Y2H_COST_CHUNKS contiguous chunks, one workgroup each with the tree above, their sums added in chunk order by
 * a second launch: for a cost over millions of values (a char-rnn's [T*B][inputs]).  scratch: Y2H_COST_CHUNKS floats. */
enum { Y2H_COST_CHUNKS = 256 };
int y2h_train_cost_sse_chunked(const float *pred, const float *truth, float *error, float *delta, float *delta_prev, float scale,
                               long n, float *cost, float *scratch, y2h_stream s);
/* [dropout] in training mode (dropout_layer.c:38-59), forward on an activation and backward on its delta, in place:
 * x = rnd < probability ? 0 : x * scale.  x is dense NHWC [batch][hw][c]; rnd holds the layer's draws in the reference's
 * [batch][c][hw] order (hw = 1: the same order). */
int y2h_train_dropout(float *x, const float *rnd, float probability, float scale, int batch, int c, int hw, y2h_stream s);
/* update_convolutional_layer's three statements per array: updates += wd * w (skipped when wd == 0), w += rate * updates,
 * updates *= momentum */
int y2h_train_sgd(float *w, float *updates, long n, float rate, float wd, float momentum, y2h_stream s);

/* ---- training, the detector's tail (y2_train_det.hip) ----
 * The [region] head with state.train = 1 (region_layer.c:144-321, CPU branch, DOABS 1, flat softmax) and
 * backward_region_layer.  `in` is the last convolution's dense NHWC output, which IS the reference's flattened layout
 * [batch][h*w][n*(5+classes)]; out (logistic on objectness, softmax over the classes) and delta keep that layout.
 * truth is [batch][150]: at most 30 rows of x, y, w, h, class per image, ended by the first x == 0; `seen` is *net.seen
 * as the step sees it (the prior-box delta runs while it is < 12800).  delta_prev receives delta (a store: the head is
 * the first writer of the layer in front), cost[0] = pow(mag_array(delta), 2) as a fixed-order two-pass sum, stats the
 * figures the reference prints.  A truth whose cell (int)(x*w), (int)(y*h) lies outside the grid is skipped whole.
 * anchors: 2*n floats in HBM.  scratch: y2h_train_region_scratch_bytes(g) bytes, 8-byte aligned.  No atomics. */
typedef struct { int batch, h, w, n, classes, bias_match, rescore; float thresh, coord_scale, object_scale, noobject_scale, class_scale; } y2h_train_region;
typedef struct { float avg_iou, avg_class, avg_obj, avg_noobj, recall; int count, class_count; } y2h_train_region_stats;
size_t y2h_train_region_scratch_bytes(const y2h_train_region *g);
int y2h_train_region_loss(const y2h_train_region *g, const float *in, const float *anchors, const float *truth, int seen, float *out,
                          float *delta, float *delta_prev, float *cost, y2h_train_region_stats *stats, void *scratch, y2h_stream s);
/* The [detection] head of YOLOv1 with state.train = 1 (detection_layer.c:49-222) and backward_detection_layer, coords = 4.
 * in / out / delta are [batch][side*side*(5*n + classes)]: per image the cells' class scores, then their n objectness
 * values, then their n boxes.  truth is [batch][side*side][1 + classes + 4] (load_data_region): is-object (the reference's
 * int cast), the class row, then x, y, w, h.  out is the input with the optional per-cell class softmax; every delta entry
 * is written (no memset); delta_prev receives delta (add == 0) or has it added; cost[0] = pow(mag_array(delta), 2) as a
 * fixed-order two-pass sum; stats are the figures the reference prints, summed in double in a fixed order and divided as in
 * its printf (NaN when count == 0).  An object cell for which no box wins (every IoU 0 or NaN and every rmse >= 20 or NaN), or
 * for which forced names box 1 of a one-box head, makes the reference go on with entries that are not the cell's (or not
 * the array's): here that cell keeps its no-object and class deltas and adds nothing to avg_iou, avg_obj and count.
 * random=1 (a draw of rand() per object cell) is not implemented: the trainer refuses it.
 * scratch: y2h_train_detection_scratch_bytes(g) bytes, 8-byte aligned.  No atomics. */
typedef struct { int batch, side, n, classes, softmax, sqrt, rescore, forced; float coord_scale, object_scale, noobject_scale, class_scale; } y2h_train_detection;
typedef struct { float avg_iou, avg_cat, avg_allcat, avg_obj, avg_anyobj; int count; } y2h_train_detection_stats;
size_t y2h_train_detection_scratch_bytes(const y2h_train_detection *g);
int y2h_train_detection_loss(const y2h_train_detection *g, const float *in, const float *truth, float *out, float *delta,
                             float *delta_prev, int add, float *cost, y2h_train_detection_stats *stats, void *scratch, y2h_stream s);
/* [route] on dense NHWC tensors of `pixels` = batch*h*w pixels: forward copies the source's c channels to channels
 * off .. off+c-1 of the route's ldc; backward stores (add == 0) or adds that slice of the route's delta to the source's */
int y2h_train_route_forward(const float *src, int c, float *dst, int ldc, int off, long pixels, y2h_stream s);
int y2h_train_route_backward(const float *droute, int ldc, int off, float *dsrc, int c, long pixels, int add, y2h_stream s);
int y2h_train_add(float *dst, const float *src, long n, y2h_stream s);                      /* dst += src */
/* backward of a non-reverse [reorg] whose input is h x w x c (reorg_layer.c:92): the exact inverse of y2h_reorg(reverse = 0),
 * an assignment.  dy is dense NHWC [h/stride][w/stride][c*stride*stride], dx dense NHWC [h][w][c]. */
int y2h_train_reorg_backward(const float *dy, float *dx, int batch, int h, int w, int c, int stride, y2h_stream s);

/* ---- training, [rnn] (y2_train_rnn.hip): the per-step parts of back-propagation through time ----
 * Tensors are [T][B][C], rows step-major; a group is one step's B rows.  Every sum has one fixed order; no atomics.
 *   bn_stats   mean / variance [T][C], each over its own group (variance / (B-1), B >= 2), then the rolling statistics
 *              rolling = keep * rolling + take * new once per step in step order
 *   bn_apply   y2h_train_bn_apply with the group's own mean / variance
 *   delta      backward_connected_layer up to its products, group by group, in place on delta: gradient_array on `out`, the
 *              group's bias sum -> bias_steps[T][C] (and sum delta * x_norm -> scale_steps), then with mean != NULL scale_bias,
 *              mean_delta, variance_delta and normalize_delta over the group's B rows.  mean / variance are ONE row [C] used
 *              for every group (the reference's backward reads the last step's); mean_delta / variance_delta [C] receive
 *              group 0's, which is what the reference's arrays hold after its loop.
 *   sum_steps  dst[c] += steps[T-1][c] + ... + steps[0][c], added one by one in that order
 *   combine    dst = (0 + a) + b */
int y2h_train_rnn_bn_stats(const float *x, int T, int B, int C, float *mean, float *variance, float *rolling_mean,
                           float *rolling_variance, float keep, float take, y2h_stream s);
int y2h_train_rnn_bn_apply(float *y, float *x, float *x_norm, const float *mean, const float *variance, const float *scales,
                           const float *biases, int act, int T, int B, int C, y2h_stream s);
/* one step of the self sub-layer behind its product y [B][C], one launch: bn_stats (T = 1), bn_apply and
 * next = (0 + proj) + y; mean == NULL: y = act(y + bias) only (x, x_norm, variance, the rolling pair and scales unused) */
int y2h_train_rnn_step_finish(float *y, float *x, float *x_norm, float *mean, float *variance, float *rolling_mean,
                              float *rolling_variance, float keep, float take, const float *scales, const float *biases, int act,
                              int B, int C, const float *proj, float *next, y2h_stream s);
/* The fused step kernels of the self sub-layer.  fits: the rule -- B <= 128 rows (four 32-row tiles of one matrix-core
 * accumulator each in a 16-wave workgroup that owns 32 columns and all rows), the LDS tiles within a CU's 160 KB, the backward
 * partials (ws_bytes = ceil(hidden / 32) * B * hidden floats) within 256 MiB.  Host arithmetic, no GPU.
 * forward: y = state x w^T on the fp32 matrix cores and everything y2h_train_rnn_step_finish does, ONE launch.
 * backward: everything y2h_train_rnn_delta does for one group (T = 1), and with dprev != NULL  dprev += delta x w: each
 * workgroup's 32 outputs give a partial in ws, a second launch adds the partials in range order.  Two launches. */
int y2h_train_rnn_fused_fits(int B, int hidden);
size_t y2h_train_rnn_fused_ws_bytes(int B, int hidden);
int y2h_train_rnn_fused_forward(const float *state, const float *w, float *y, float *x, float *x_norm, float *mean, float *variance,
                                float *rolling_mean, float *rolling_variance, float keep, float take, const float *scales,
                                const float *biases, int act, int B, int H, const float *proj, float *next, y2h_stream s);
int y2h_train_rnn_fused_backward(const float *out, float *delta, const float *x, const float *x_norm, const float *scales,
                                 const float *mean, const float *variance, int act, int B, int H, const float *w, float *bias_step,
                                 float *scale_step, float *mean_delta, float *variance_delta, float *dprev, float *ws, y2h_stream s);
int y2h_train_rnn_delta(const float *out, float *delta, const float *x, const float *x_norm, const float *scales, const float *mean,
                        const float *variance, int act, int T, int B, int C, float *bias_steps, float *scale_steps,
                        float *mean_delta, float *variance_delta, y2h_stream s);
int y2h_train_rnn_sum_steps(const float *steps, int T, int C, float *dst, y2h_stream s);
int y2h_train_rnn_combine(const float *a, const float *b, float *dst, long n, y2h_stream s);
int y2h_train_rnn_add_transposed(float *dst, const float *src, int outputs, int inputs, y2h_stream s);   /* dst[o][k] += src[k][o] */
/* get_rnn_data (rnn.c:86-114) on the device: tok is [B][T + 1] bytes in HBM, every one below C (the caller checked); x and y
 * are [T][B][C]: x[t*B + b] is the one-hot of tok[b][t], y[t*B + b] of tok[b][t + 1].  Every element is written. */
int y2h_train_rnn_onehot(const unsigned char *tok, int T, int B, int C, float *x, float *y, y2h_stream s);

/* ---- dreaming (y2_dream.hip): the picture side of nightmare.c's optimize_picture / run_nightmare ----
 * One resample is crop_image(src, cx, cy, cw, ch) -> resize_image(., ow, oh) -> crop_image(., px, py, ow, oh), both crops
 * repeating edge pixels (constrain_int), with flip_image on the source (src_flip) or on the result (dst_flip) and either
 * layout ([c][h][w] or [h][w][c]) on either end.  Two launches; tmp holds y2h_dream_resample_tmp_floats(r) floats.  The
 * values are formed by the fp32 expressions of y2h_resize_chw in its order, nothing contracted. */
typedef struct {
    int c;
    int sh, sw, src_nhwc, src_flip;      /* the source */
    int cx, cy, ch, cw;                  /* the crop in front of the resize */
    int oh, ow;                          /* the resize */
    int px, py;                          /* the crop behind it */
    int dst_nhwc, dst_flip;              /* the result */
} y2h_dream_resample;
size_t y2h_dream_resample_tmp_floats(const y2h_dream_resample *r);
int y2h_dream_resample_run(const y2h_dream_resample *r, const float *src, float *tmp, float *dst, y2h_stream s);
/* Deterministic moments: block b sums chunk b of Y2H_DREAM_CHUNK values (16 per thread in index order, then a fixed tree),
 * the chunk sums are added in chunk order by the same tree; the variance is a second pass about the mean.  `partials`
 * holds 2 * y2h_dream_chunks(n) floats; stat[0] = mean, stat[1] = variance (/n).  No floating-point atomics.
 *   loss    nightmare.c:23-32 calculate_loss: delta[i] = output[i] where (double)output[i] > mean + thresh*sqrt(var), else 0;
 *           *selected = how many were kept (output and delta may be any layout: the rule is per element)
 *   apply   norm: out = (out - mean) / (float)sqrt(var) (utils.c:482, no epsilon: 0/0 stays NaN); then
 *           picture = constrain(picture + rate * out) with constrain_image's two tests, which a NaN passes */
#define Y2H_DREAM_CHUNK 4096
int y2h_dream_chunks(long n);
int y2h_dream_loss(const float *output, float *delta, long n, float thresh, float *partials, float *stat, int *selected, y2h_stream s);
int y2h_dream_apply(float *picture, const float *out, long n, float rate, int norm, float *partials, float *stat, y2h_stream s);
/* image.c:1481 rotate_image about (w/2., h/2.) with bilinear_interpolate; cos(rad) and sin(rad) come from the host's libm as
 * doubles, the coordinates are formed in double and rounded to float as the C expression does.  src != dst. */
int y2h_dream_rotate(const float *src, float *dst, int c, int h, int w, double cos_rad, double sin_rad, y2h_stream s);

/* ---- Go (y2_go.hip): go.c's predict_move views, rules and generate_move's decision, batched ----
 * Boards are [n][361] floats holding exactly 0, 1 or -1, row-major (board[row*19+col]); players are +1 / -1; a ko string
 * is board_to_string's 91 bytes (go.c:75-90); legal / suicide maps are bytes, liberties ints.
 * y2h_go_views   x[(b*V+v)][361], V = multi ? 8 : 1: view v of board b is rotate_image_cw(board, v) -- one turn is
 *                new[r][c] = old[c][18-r] (image.c:1035-1054) -- then flip_image (columns) when v >= 4; players[b] < 0
 *                negates the board first (flip_board).
 * y2h_go_merge   move[b] = row 0, += rows 1..7 un-flipped (v >= 4) and turned by -v, in that order in fp32, x 0.125
 *                (go.c:265-284); with multi = 0 row 0 alone; then 0 wherever boards[b] is non-zero.  rows are V*n rows of
 *                ld floats.
 * y2h_go_rules   per position: liberties as calculate_liberties (go.c:188), legal as legal_go(board, ko, player, r, c)
 *                (go.c:338: occupied points and a move whose packed result equals ko are illegal, suicide is not), suicide
 *                as suicide_go (go.c:326).  ko may be NULL (all strings zero); any output may be NULL.  One workgroup per
 *                position, integers in LDS, no global atomics: the same bytes on every run.
 * y2h_go_apply   move_go(board, player, move / 19, move % 19) in place where 0 <= moves[b] < 361, then board_to_string into
 *                strings[b] (or NULL).
 * y2h_go_play    one ply of self_go (go.c:801-822) for the games with alive[b]: index[b] < 0 clears alive[b]; otherwise the
 *                record (row, column, the board packed from the mover's side) lands at records[b][counts[b]++] ([n][max_moves]
 *                [93]), the move is made and the new board is packed into ko[b] ([n][91]).
 * y2h_go_pick    generate_move from go.c:362 on: illegal points zeroed, top_k's insertion rule for the five best, the
 *                threshold (go.c:370), max_index, sample_array with u[b] as its one uniform; index[b] = -1 when the arg-max
 *                is suicide, else the sample, or the arg-max when the sample is suicide.  kept (or NULL) receives the
 *                thresholded array, before sample_array scales it.
 * y2h_go_argmax  max_index per row (the first maximum).
 * y2h_go_decode  item i from record pick[i] (NULL: i) of 93-byte records: string_to_board of bytes 2..92.  With labels (the
 *                training loader, random_go_moves go.c:92-115): the one-hot label at (row, col), the board cleared there,
 *                flip_image when flip[i], then rotate_image_cw(rot[i]), on both.  Rows and columns must lie in 0..18. */
int y2h_go_views(const float *boards, const int *players, int n, int multi, float *x, y2h_stream s);
int y2h_go_merge(const float *rows, int ld, const float *boards, int n, int multi, float *move, y2h_stream s);
int y2h_go_rules(const float *boards, const unsigned char *ko, const int *players, int n, int *liberties, unsigned char *legal,
                 unsigned char *suicide, y2h_stream s);
int y2h_go_apply(float *boards, const int *players, const int *moves, int n, unsigned char *strings, y2h_stream s);
int y2h_go_play(float *boards, unsigned char *ko, int player, const int *index, int *alive, unsigned char *records,
                int *counts, int max_moves, int n, y2h_stream s);
int y2h_go_pick(const float *move, int ld, const unsigned char *legal, const unsigned char *suicide, int n, float thresh,
                const float *u, int *index, float *kept, y2h_stream s);
int y2h_go_argmax(const float *move, int ld, int n, int *index, y2h_stream s);
int y2h_go_decode(const unsigned char *records, const int *pick, const int *flip, const int *rot, int n, float *boards,
                  float *labels, y2h_stream s);

#ifdef __cplusplus
}
#endif
#endif /* Y2_HIP_H */
