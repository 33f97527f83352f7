/* Internal declarations shared by the host C sources of libsr_yolo2.so. */
#ifndef Y2_INTERNAL_H
#define Y2_INTERNAL_H

#include <stddef.h>
#include <stdint.h>
#include "sr_yolo2.h"
#include "y2_hip.h"

/* per-layer device-side state (layer.dev) */
typedef struct y2_ldev {
    struct y2_engine *eng;
    int index;
    /* where this layer's activations live: NHWC, `ld` floats between pixels */
    float *out;
    int out_ld;
    float *out_alloc;          /* allocation owned by this layer, NULL when the output sits in another buffer */
    size_t out_floats;
    int placed_in;             /* index of the [route] layer whose buffer holds this output, or -1 */
    int alias_of;              /* [route] with one input / [cost]: index of the layer whose output is reused, or -1 */
    unsigned copy_mask;        /* [route]: bit k set -> input k needs a copy kernel (could not be placed) */
    /* convolution parameters inside the weight arena */
    size_t off_w_packed, off_w_ref, off_bias, off_mean, off_scale, off_rinv;
    int has_w_ref;
    int uses_mfma;
    int form;                  /* conv: the Y2_FORM_* it runs in (y2_plan.c plan_conv_forms); what off_w_packed holds, the scratch and
                                  the entry point that go with a form are its row of y2_conv_forms */
    int fused_pool;           /* conv: the following 2x2/2 maxpool runs in this conv's epilogue */
    int fused_into;            /* maxpool: index of the conv that computes it, or -1 */
    int out_half;              /* this layer's activations are IEEE half (fp16 mode), out_ld counts halves */
    size_t off_alpha, off_beta; /* fp16 mode: folded batch-norm, y = act(acc*alpha + beta) */
    char kname[80];
    int tile_bm, tile_bn, ksplit;   /* measured tile choice (y2_set_autotune), 0 = the host's cost model */
    int conn_ranges;           /* fp16 mode [connected]: K ranges of connected_f16, 0 = the layer does not run it */
    /* region */
    float *d_anchors;
    int *d_tree_block, *h_tree_block;  /* the head's tree tables in one allocation and their host copy (y2_plan.c plan_tree_tables) */
    size_t tree_block_ints;
    int *d_tree_parent, *d_tree_gsize, *d_tree_goff, *d_map;     /* the d_tree_* tables point into d_tree_block */
    int *d_tree_order, *d_tree_loff;   /* nodes by depth level (only when parents precede children) */
    int tree_levels;
    /* every node's group (tree.group), and for [softmax] tree= the leaf flags hierarchy_predictions(.., only_leaves = 1) reads;
     * h_tree_leaf is the host copy of what d_tree_leaf holds, so a change_leaves between two calls is seen and sent up once */
    int *d_tree_group, *d_tree_leaf, *h_tree_leaf;
    float *d_tree_best;                /* [2 * boxes]: the region layer's (score | class) per box for y2h_detect_tree_chain, or NULL */
    int tree_best_valid;               /* the last forward filled d_tree_best (it does unless the detection chain overlaps the next forward) */
    float *d_region;           /* [batch][outputs] flattened region output */
    /* classifier tail */
    float *d_flat;             /* avgpool / softmax output [batch][outputs] */
    /* [crop] in front of a few-channel convolution: a second copy of the window with a zero border of halo_px
     * pixels ([batch][out_h+2p][out_w+2p][out_c]), which is what the first-layer / stem kernels read */
    float *d_halo;
    int halo_px;
    float *d_bin;              /* xnor=1 convolution: its input binarized to +-1 ([batch][h][w][c], contiguous) */
    const char *kernel;        /* name for profiles */
    /* [rnn] / [gru]: the sub-layers packed into the arena as three dense blocks, [n][k] weights each
     * (rnn: input, self, output; gru: input z|r|h stacked by rows, state z|r, state h); `form` is the Y2_REC_* the block
     * runs in, decided once per plan (y2_rec.c rec_form) */
    struct { size_t off_w, off_bias, off_mean, off_scale, off_rinv; int n, k, bn; ACTIVATION act; int form; } rd[3];
    float *d_state;            /* [B][hidden]: persists across forwards; zeroed at plan build and by reset_rnn_state */
    float *d_proj;             /* [T*B][hidden | 3*outputs]: every step's input projections, one GEMM per forward */
    float *d_hist;             /* rnn: [T*B][hidden] the states of this forward, read by the output GEMM */
    float *d_zf;               /* gru: z and f of the current step, [2][B][outputs] */
    float *d_tmp;              /* matrix-core step form: the step's dense values, [B][2*outputs] */
} y2_ldev;

/* How a convolution runs (y2_ldev.form, decided by y2_conv_layer_form): the direct kernels of y2h_conv_forward, Winograd
 * F(2x2,3x3) as three launches with U[16][n][c] in the filter slot, the same with the GEMM split into three bf16 planes
 * (y2_split_rule.h), the fused stationary Winograd kernel with U in its register order (y2_winos_rule.h), or the direct
 * kernel on the bf16 matrix cores with the split filters in its streaming order (y2_splitd_rule.h). */
enum { Y2_FORM_DIRECT = 0, Y2_FORM_WINO, Y2_FORM_WINOX, Y2_FORM_WINOS, Y2_FORM_SPLITD, Y2_FORM_COUNT };
/* What depends on the form, one row per form (y2_arena.c).  The direct row holds its workspace query alone: its filter
 * slot depends on the storage mode, its packer on the network and its entry point on the strict flag, so the sites that
 * find a NULL there spell those out. */
typedef struct y2_conv_form {
    uint64_t sig;                                        /* mixed into the arena signature; 0: nothing is mixed */
    size_t (*slot_bytes)(const layer *l);                /* what the form keeps at off_w_packed ... */
    void (*pack)(void *slot, const layer *l);            /* ... and how the host weights get there */
    size_t (*workspace_bytes)(const y2h_conv *c);        /* scratch in the shared workspace; NULL: none */
    int (*forward)(const y2h_conv *c, y2h_stream s);
} y2_conv_form;
extern const y2_conv_form y2_conv_forms[Y2_FORM_COUNT];

/* how a recurrent layer's dense products run (y2_rec.c rec_form) */
enum { Y2_REC_REF = 0, Y2_REC_SKINNY = 1, Y2_REC_MFMA = 2 };

/* network.h:15-17 and the fields of struct network that get_current_rate reads (network.c:48-79); kept here because the
 * layout of struct network is part of the ABI */
enum { Y2_LR_CONSTANT = 0, Y2_LR_STEP, Y2_LR_EXP, Y2_LR_POLY, Y2_LR_STEPS, Y2_LR_SIG, Y2_LR_RANDOM };
typedef struct {
    int policy, step, burn_in, num_steps, adam;
    float scale, gamma, power;
    int *steps;
    float *scales;
} y2_lr_schedule;

typedef struct y2_engine {
    int device;
    y2h_stream stream;
    int strict;
    int timing;
    int fusion, built_fusion;  /* conv+maxpool fusion enabled / state of the current plan */
    int half, built_half;      /* fp16 storage requested (y2_set_half) / state of the current plan */
    int autotune, built_autotune; /* measure the conv tile shapes at plan time (y2_set_autotune) */
    int in_form;               /* Y2_IN_*: how the network input reaches layer 0 (y2_plan.c choose_input_form) */
    const float *cur_input;    /* the NCHW input of the forward pass being enqueued (Y2_IN_NCHW, a flat recurrent input) */
    int in_halo_px;            /* the border's width in pixels: 1 for the 3x3 first-layer kernels, the padding for the stem kernel */
    /* hipGraph replay of the forward launch sequence (y2_set_graph): recorded for one input pointer, dropped with the plan */
    y2h_event ev_out;          /* recorded behind the output copy of y2_output_enqueue */
    int out_pending;
    y2h_event ev_det;          /* recorded behind the D2H copies of y2_detect_enqueue */
    /* y2_set_detect_overlap: decode / NMS / compaction of batch i on their own stream beside the forward pass of batch i+1 */
    int det_overlap;
    y2h_stream det_stream;
    y2h_event ev_fwd;          /* recorded on `stream` behind the forward pass whose region output the detect chain reads */
    int det_pending;           /* 1: wait for ev_det in y2_detect_fetch, 2: already fetched synchronously */
    int graph_on;
    uint64_t graph_params;     /* hash of the layer fields a recording bakes in that callers may write (softmax temperature) */
    y2h_graph graph;           /* the graph in use (one of graphs[]) */
    const float *graph_src;
    y2h_graph graphs[4];       /* recorded forward passes by input pointer (a double-buffered feed alternates between two) */
    const float *graph_srcs[4];
    int graph_next;            /* slot the next recording replaces */
    /* plan state */
    int built;
    int built_batch, built_w, built_h, built_strict;
    int weights_dirty;         /* host weights changed since the last upload */
    int weights_external;      /* arena filled from outside (broadcast) */
    unsigned long weights_gen; /* counts the changes of the host weights (load_weights, denormalize, a trainer's sync): what a
                                  holder of packed copies of its own (y2_dream.c) compares against */
    /* weight arena */
    unsigned char *arena;
    size_t arena_bytes;
    size_t arena_need;         /* bytes the layout of the plan being built asks for (y2_arena_layout) */
    int arena_pending;         /* the arena was laid out for a fill from outside (y2_weights_arena) that has not happened yet */
    int class_counts_zeroed;   /* d_class_counts is all zero (the three-launch detect chain keeps it so) */
    int capturing;             /* inside the hipGraph capture of a forward pass (no cross-stream waits may be recorded) */
    uint64_t arena_sig;        /* hash of the per-layer offsets / forms the arena was laid out with (0: none yet) */
    /* io buffers */
    float *d_in_nchw, *d_in_nhwc;
    size_t in_floats;
    float *d_out_nchw;         /* staging when the output layer is image-like */
    unsigned char *d_u8;       /* y2_detect_u8: raw frames, float planes, resize scratch (grow-only) */
    float *d_planes, *d_rtmp;
    size_t u8_cap, planes_cap, rtmp_cap;
    /* y2_ingest_regions: descriptor table + packed region rows, staged in pinned memory and sent up in one copy */
    unsigned char *h_reg_stage, *d_reg;  /* both grow-only */
    size_t reg_stage_cap, reg_cap;
    y2h_event ev_reg;                    /* recorded behind that copy: the staging buffer may be refilled after it */
    int reg_pending;
    float *d_ws;               /* split-K scratch shared by all conv layers */
    size_t ws_bytes;
    float *h_out;              /* what network_predict returns; allocated at parse time like the reference's
                                  l.output (callers copy `layer` structs early), pinned once a GPU is in use */
    size_t out_floats;
    size_t h_out_cap;          /* floats allocated behind h_out */
    int h_out_pinned;          /* h_out came from hipHostMalloc (a GPU was present at parse time): predict copies straight into it */
    float *h_out_stage;        /* pinned (hipHostMalloc) landing buffer of the PIPELINED output copy (y2_output_enqueue / _fetch: the
                                  caller may still read h_out while the next copy flies) and of hosts without pinned h_out;
                                  heap memory is never handed to the GPU: registering h_out in place
                                  (hipHostRegister) made the runtime treat a pageable buffer that starts in the page behind
                                  it as part of the registration -- the next weight upload from such a buffer faulted */
    size_t h_out_stage_cap;
    int out_layer;
    /* decode / nms buffers for the output region layer */
    float *d_boxes, *d_probs, *d_probs_nms, *d_records;
    int *d_counts;
    int *d_class_counts;       /* [batch][classes] non-zero scores (NMS skips empty classes) */
    float *d_best;             /* [2][batch][total] best score / class per box */
    float *d_mean_ring;        /* y2_detect_mean: three region-output slots + their average (batch 1) */
    size_t mean_els;
    int mean_index;
    float *h_records;
    int *h_counts;
    int det_cap;               /* records per image */
    int det_batch, det_total, det_classes;
    /* pinned, multi-buffered host feed (y2_feed.c) */
    int feed_slots;
    size_t feed_bytes;
    void **feed_host, **feed_dev;
    y2h_event *feed_up, *feed_done;    /* per slot: H2D finished / the forward that read the device copy was enqueued and ran */
    int *feed_used;                    /* per slot: feed_done has been recorded at least once */
    y2h_stream feed_stream;            /* copies run here, next to the engine stream's kernels */
    /* text generation / scoring (y2_chargen.c), grow-only: tokens [steps][B], one uniform per draw, one probability per
     * scored row, the rows a caller asked to see */
    int *d_gen_tok;
    float *d_gen_u, *d_gen_p, *d_gen_probs;
    size_t gen_tok_cap, gen_u_cap, gen_p_cap, gen_probs_cap;
    /* classifier views (y2_tta.c), grow-only: one pinned staging buffer (tables + the block's source planes) and one HBM
     * arena (the same, the resized copies, the resize scratch, the block's accumulators) */
    unsigned char *h_tta, *d_tta;
    size_t h_tta_cap, d_tta_cap;
    struct y2_depth_state *depth;      /* the depth stage's planes and scratch (y2_depth.c), NULL until the first upload */
    struct y2_kcf_state *kcf;          /* the KCF trackers (y2_kcf.c), NULL until the first y2_kcf_init */
    struct y2_go_state *go;            /* the Go entries' HBM and pinned blocks (y2_go.c), NULL until the first call */
    /* timing */
    y2h_event *ev;             /* n+1 events */
    int n_ev;
    int n_layers;
    /* training (y2_train.c): the [net] section's learning-rate schedule, and the trainer once y2_train_prepare built it */
    y2_lr_schedule lr;
    int train_precision;       /* Y2_TRAIN_FP32 / _BF16X3 / _BF16: the kernel of the three convolution products of a step; it lives
                                  here and not in the trainer, so it outlasts y2_train_free and every new y2_train_prepare */
    struct y2_trainer *trainer;
    float aug_hue, aug_saturation, aug_exposure;   /* [net] hue / saturation / exposure (parser.c:532-534): what y2_net_augment reports */
    struct y2_dream *dream;    /* optimize_picture's cached context (y2_dream.c), NULL until its first call */
    int aug_min_crop, aug_max_crop;                /* [net] min_crop / max_crop / angle / aspect (parser.c:527-531): y2_net_augment_classifier */
    float aug_angle, aug_aspect;
} y2_engine;

/* How the network input (fp32 NCHW) reaches layer 0: a plain NHWC copy; an NHWC copy with a zero border of in_halo_px
 * pixels (no tap bounds tests in the first-layer / stem kernels); a half [b][h+2][w+2][4] copy for the fp16 first-layer
 * kernel; or no copy at all, the first-layer kernel reads the NCHW planes itself. */
enum { Y2_IN_NHWC = 0, Y2_IN_NHWC_HALO = 1, Y2_IN_NHWC4_HALO_F16 = 2, Y2_IN_NCHW = 3 };
/* what each form means for layer 0's descriptor and for the engine's NHWC input buffer (y2_plan.c y2_input_form) */
typedef struct { size_t floats; int ldx, x_halo, x_f16, x_nchw; } y2_in_form;

/* error handling: mode 0 = the reference's contract (message + exit), 1 = record and return */
void y2_fail(const char *fmt, ...);
int y2_error_mode(void);
int y2_failed(void);           /* and clear */

/* call, report a failure, and then: return -1 / return / release scratch buffers at `cleanup:` */
#define HIPCALL(expr, text, onfail) do { int rc_ = (expr); if (rc_ != 0) { y2_fail("%s failed (%d): %s", text, rc_, y2h_last_error()); onfail; } } while (0)
#define HIP_OR_ERR(expr) HIPCALL(expr, #expr, return -1)
#define HIP_OR_RET(expr) HIPCALL(expr, #expr, return)
#define HIP_OR_CLEANUP(expr) HIPCALL(expr, #expr, goto cleanup)

/* a 256-byte aligned pointer that stands in for arena / buffer addresses in shape queries made before they exist */
#define Y2_ALIGNED_STANDIN ((float *)(uintptr_t)256)

static inline y2_ldev *ld_of(const layer *l) { return (y2_ldev *)l->dev; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int is_recurrent(const layer *l) { return l->type == RNN || l->type == GRU; }

/* engine (y2_engine.c) */
y2_engine *y2_engine_of(const network *net);
int y2_engine_create(network *net);
void y2_engine_destroy(network *net);
void y2_engine_invalidate(network *net);
void y2_engine_host_output(network *net);
void y2_drop_graphs(y2_engine *e);
int y2_enqueue_forward(network *net, const float *d_input_nchw);
int y2_activate_after(y2_engine *e, ACTIVATION a, float *y, int ld, long rows, int n);
int y2_engine_forward(network *net, const float *d_input_nchw);
int y2_engine_fetch_output(network *net);
int y2_output_device(network *net, const float **rows);
const char *y2_hierarchy_refusal(const network *net, char *buf, size_t cap);
float *y2_predict_hierarchy(network *net, float *input, int only_leaves);
int y2_hierarchy_leaves(network *net);
int y2_hierarchy_device(network *net, float *rows, int nrows, int only_leaves, const int *d_row_mask);
int y2_ingest_u8_device(network net, const unsigned char *d_frames, int h, int w, int c, int step, int swap_rb, int letterbox);

/* plan (y2_plan.c) */
int y2_engine_build(network *net);
void y2_free_plan(network *net);
int y2_softmax_tree_check(const network *net);
int y2_act_code(ACTIVATION a);
int y2_act_in_kernel(ACTIVATION a);
int y2_act_for_kernel(ACTIVATION a);
int y2_flat_input(const network *net);
int y2_producer_of(const network *net, int i);
int y2_is_flat(const network *net, int i);
int y2_half_weights(const network *net, int i);
void y2_input_form(const network *net, y2_in_form *f);
void y2_input_view(const network *net, int i, const float **x, int *ldx);
void y2_conv_desc(const network *net, int i, y2h_conv *c, const float *x, int ldx);
int y2_conv_layer_form(const y2h_conv *c, int fused_pool, char *name, size_t name_len);   /* y2_conv_form_of, then the direct split rule */
int y2_conv_form_of(const y2h_conv *c, int fused_pool, char *name, size_t name_len);   /* host arithmetic only */

/* weight arena (y2_arena.c) */
void y2_bn_slots(size_t *off, int n, size_t *mean, size_t *scale, size_t *rinv);
void y2_fill_rinv(double *dst, const float *var, int n);
void y2_arena_layout(network *net);
int y2_arena_commit(network *net);
int y2_upload_weights(network *net);

/* [rnn] / [gru] (y2_rec.c) */
int y2_rec_hidden(const layer *l);
int y2_rec_plan(network *net, int i);
size_t y2_rec_layout(y2_ldev *d, const layer *l, size_t off);
void y2_rec_pack(unsigned char *host, const y2_ldev *d, const layer *l);
size_t y2_rec_workspace_bytes(const network *net);
int y2_rec_forward(network *net, int i, const float *x);

/* text generation / scoring (y2_chargen.c) */
void y2_chargen_free(y2_engine *e);

/* regions (y2_detect.c) and the depth stage behind them (y2_depth.c) */
int y2_ingest_regions_far(const char *who, network net, const y2_region *items, int n, const float *far_m, int swap_rb, int letterbox);
void y2_region_rect(const y2_region *it, int *x, int *y, int *rw, int *rh);
int y2_regions_check(const char *who, network net, const y2_region *items, int n, int letterbox);
int y2_detect_chain_enqueue(network net, float thresh, float nms);
int y2_detect_chain_fetch(network net, y2_det *dets, int *counts, int max_per_item, int items);
void y2_fill_object(object *o, const y2_det *d, char **names, int classes);
int y2_depth_filter_check(const char *who, network net, const y2_region *items, int n, const float *far_m);
const unsigned char *y2_depth_plane8(const y2_engine *e, int *W);
const unsigned short *y2_depth_plane_grasp(const y2_engine *e);
void y2_depth_free(y2_engine *e);
void y2_kcf_free_engine(y2_engine *e);            /* the KCF trackers (y2_kcf.c) */
void y2_go_free_engine(y2_engine *e);             /* the Go entries' blocks (y2_go.c) */

/* training (y2_train.c) */
int y2_train_is_dirty(const network *net);     /* steps ran since the masters last reached the host arrays */
int y2_train_sync_if_dirty(network *net);      /* a trained network's masters reach the host arrays before they are read */
void y2_lr_parse(list *options, y2_lr_schedule *lr);
int y2_train_precision_env(int *mode);            /* Y2_TRAIN_PRECISION -> *mode (untouched when unset); -1 and y2_fail for an unknown word */

/* dreaming (y2_dream.c) */
void y2_dream_free_cached(y2_engine *e);

/* the detection loader's host half (y2_aug.c), device-free */
int y2_aug_check(const char *who, const y2_aug_item *items, int n);        /* every refusal that reads only the items */
void y2_aug_rect(const y2_aug_item *it, int *x0, int *y0, int *rw, int *rh);
size_t y2_aug_pack_bytes(const y2_aug_item *items, int n);
void y2_aug_pack(const y2_aug_item *items, int n, int net_w, int net_h, y2h_aug *desc, unsigned char *pixels);
/* the classifier loader's: the same three steps for y2_aug_cls_item (size = the output's edge) */
int y2_aug_cls_check(const char *who, const y2_aug_cls_item *items, int n);
void y2_aug_cls_rect(const y2_aug_cls_item *it, int size, int *x0, int *y0, int *rw, int *rh);
size_t y2_aug_cls_pack_bytes(const y2_aug_cls_item *items, int n, int size);
void y2_aug_cls_pack(const y2_aug_cls_item *items, int n, int size, y2h_aug_cls *desc, unsigned char *pixels);
/* the two halves of y2_aug_cls_pack, for a caller that sizes its buffer between them: the table (and the bytes its
 * rectangles take), then the copy */
size_t y2_aug_cls_describe(const y2_aug_cls_item *items, int n, int size, y2h_aug_cls *desc);
void y2_aug_cls_copy(const y2_aug_cls_item *items, int n, const y2h_aug_cls *desc, unsigned char *pixels);

/* cfg helpers shared with other files */
char *y2_fgetl(FILE *fp);
void y2_strip(char *s);
int y2_out_layer(const network *net);

#endif
