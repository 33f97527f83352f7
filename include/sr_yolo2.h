/*
 * sr_yolo2.h -- drop-in C API of the MI355X-native YOLOv2 / Darknet forward engine.
 *
 * This header declares, with the reference's own names, argument meaning and
 * error behaviour, the entry points a caller of the reference's forward path
 * binds.  Each declaration cites the reference
 * interface it replaces (paths relative to src_yolo2/ of
 * NidhiMishra/SR_object_detection).  The thin headers network.h, parser.h,
 * layer.h, box.h, region_layer.h, cuda.h, image.h, utils.h, option_list.h,
 * tree.h and test_detector.h next to this file simply include it, so the
 * Kinect / CLI callers keep their #include lines.
 *
 * Differences a caller can observe (all deliberate):
 *   - `layer` and `network` keep every field the forward-path callers read
 *     (yolo_v2_class.cpp:64-76,202-216; KinectUtil.cpp:85; detector.c:568-576)
 *     but drop the training-only members, and their layout no longer depends
 *     on -DGPU / -DCUDNN (layer.h:205-263, network.h:63-66): device state
 *     hangs off one opaque pointer.
 *   - there is no CPU compute path in this library: network_predict always
 *     runs on the GPU selected by net.gpu_index (>= 0).  gpu_index < 0, which
 *     selects the CPU path in the reference (network.c:461), is an error here.
 *   - only the last non-[cost] layer has a host `output` buffer; other layers'
 *     activations stay in HBM (use y2_pull_layer_output to inspect them).
 *   - set_batch_network may grow the batch (the reference overflows its
 *     parse-time buffers); buffers are re-planned lazily.
 *   - net.seen is 8 bytes, so a version >= 0.2 .weights header no longer
 *     overruns it (parser.c:1027-1029 vs network.c:137).
 */
#ifndef SR_YOLO2_H
#define SR_YOLO2_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums: names and order are part of the ABI callers compile against ---- */
/* activations.h:7-9 */
typedef enum {
    LOGISTIC, RELU, RELIE, LINEAR, RAMP, TANH, PLSE, LEAKY, ELU, LOGGY, STAIR, HARDTAN, LHTAN
} ACTIVATION;

/* layer.h:13-38 */
typedef enum {
    CONVOLUTIONAL, DECONVOLUTIONAL, CONNECTED, MAXPOOL, SOFTMAX, DETECTION, DROPOUT, CROP, ROUTE, COST,
    NORMALIZATION, AVGPOOL, LOCAL, SHORTCUT, ACTIVE, RNN, GRU, CRNN, BATCHNORM, NETWORK, XNOR, REGION, REORG, BLANK
} LAYER_TYPE;

/* layer.h:40-42 */
typedef enum { SSE, MASKED, SMOOTH } COST_TYPE;

/* tree.h:4-14 */
typedef struct {
    int *leaf;
    int n;
    int *parent;
    int *group;
    char **name;
    int groups;
    int *group_size;
    int *group_offset;
} tree;

/* box.h:4-6 */
typedef struct { float x, y, w, h; } box;

/* image.h:12-17: CHW planes, values in [0,1] */
typedef struct { int h; int w; int c; float *data; } image;

/* utils.h:14-28: what test_detector_img hands to the Kinect pipeline */
typedef struct {
    float x, y;
    float w, h;
    char name[20];
    float prob;
    int objClass;
    float CameraX, CameraY, CameraZ;
    float CameraWidth, CameraHeight;
    unsigned char flagBelong2Person;
    float boxRGB[3];
    int bodyId;
} object;

/* list.h / option_list.h: key=value lists returned by read_data_cfg */
typedef struct node { void *val; struct node *next; struct node *prev; } node;
typedef struct list { int size; node *front; node *back; } list;
typedef struct { char *key; char *val; int used; } kvp;

struct layer;
typedef struct layer layer;
struct network;

/* layer.h:44-264, forward-path subset.  Host-visible description of one layer. */
struct layer {
    LAYER_TYPE type;
    ACTIVATION activation;
    COST_TYPE cost_type;
    int batch_normalize;
    int batch;
    int flipped;
    int inputs, outputs;
    int h, w, c;
    int out_h, out_w, out_c;
    int n;                     /* filters | anchors | number of route inputs */
    int groups;
    int size, stride, pad;
    int reverse;
    int index;
    int binary, xnor;
    /* [region] */
    int softmax, classes, coords, classfix, log, sqrt, max_boxes, rescore, bias_match, random, absolute, truths;
    float jitter, thresh, coord_scale, object_scale, noobject_scale, class_scale;
    /* [softmax] / [cost] */
    float temperature, scale;
    int dontload, dontloadscales;
    tree *softmax_tree;
    int *map;
    int *input_layers, *input_sizes;      /* [route] */
    float *biases, *scales, *weights;     /* host copies, reference layouts ([n][c][k][k]) */
    float *rolling_mean, *rolling_variance;
    float *output;                        /* host; non-NULL only for the network's output layer */
    float *delta;                         /* always NULL (the trainer's deltas live in HBM: y2_train_pull) */
    float *cost;
    size_t workspace_size;                /* the reference's im2col bytes (convolutional_layer.c:135); informational */
    void *dev;                            /* opaque device-side state */
    /* YOLOv1 family: [detection] grid side and `forced`, [dropout] probability */
    int side, forced;
    float probability;
    /* [crop] (crop_layer.c:16-46; `scale` above holds crop_height / h for resize_crop_layer) */
    int flip, noadjust;
    float angle, saturation, exposure, shift;
    /* [rnn] / [gru] (rnn_layer.c:29-60, gru_layer.c:29-87): `batch` is B = net.batch / steps sequences, each run for
     * `steps` time steps per forward.  Every sub-layer is a host [connected] layer holding its parameters. */
    int steps, hidden, shortcut;
    struct layer *input_layer, *self_layer, *output_layer;                  /* [rnn] */
    struct layer *input_z_layer, *state_z_layer, *input_r_layer, *state_r_layer, *input_h_layer, *state_h_layer;   /* [gru] */
    /* [normalization] (normalization_layer.c:5-19): the window is `size` channels; y = x * (kappa + alpha * sum)^-beta */
    float alpha, beta, kappa;
};

/* network.h:19-67, forward-path subset */
typedef struct network {
    float *workspace;          /* always NULL: there is no im2col workspace */
    int n;
    int batch;
    int *seen;                 /* 8 bytes are allocated behind this pointer */
    int subdivisions;
    float learning_rate, momentum, decay;
    int max_batches, time_steps;
    layer *layers;
    int outputs;
    float *output;
    int inputs;
    int h, w, c;
    int gpu_index;
    tree *hierarchy;
    void *engine;              /* opaque: plan, HBM buffers, stream */
} network;

/* network.h:69-77 kept for source compatibility of callers that mention the type */
typedef struct network_state {
    float *truth;
    float *input;
    float *delta;
    float *workspace;
    int train;
    int index;
    network net;
} network_state;

/* ---- device selection (cuda.h:8,28; cuda.c:1,12) ---- */
extern int gpu_index;                          /* default device for parse_network_cfg; 0 at start-up */
void cuda_set_device(int n);

/* ---- cfg + weights (parser.h:5-11) ---- */
network parse_network_cfg(char *filename);                       /* parser.c:585 */
void load_weights(network *net, char *filename);                 /* parser.c:1084 */
void load_weights_upto(network *net, char *filename, int cutoff);/* parser.c:1009 */
void denormalize_convolutional_layer(layer l);                   /* convolutional_layer.c:321 */
void y2_denormalize_network(network *net);                       /* darknet.c:309-345 denormalize_net, conv layers */
void save_weights(network net, char *filename);                  /* parser.c:878  (version 0.1 header) */
void save_weights_upto(network net, char *filename, int cutoff); /* parser.c:822 */

/* ---- network runtime (network.h:83-127) ---- */
network make_network(int n);                                     /* network.c:132 */
void free_network(network net);                                  /* network.c:592 */
void set_batch_network(network *net, int b);                     /* network.c:308 */
int resize_network(network *net, int w, int h);                  /* network.c:322 */
float *network_predict(network net, float *input);               /* network.c:458 */
float *network_predict_gpu(network net, float *input);           /* network_kernels.cu:392 */
float *get_network_output(network net);                          /* network.c:173 */
/* rnn.c:116: zero item b's hidden state in every [rnn] / [gru] layer; b = -1 zeroes every item (an extension).
 * Recurrent networks read and write rows step-major: row t*B + b is step t of sequence b (B = net.batch / time_steps).
 * The state lives in HBM; it is zeroed when the plan is built (the first predict, set_batch_network) and by this call,
 * and nothing else touches it: every forward (network_predict, y2_forward_device, y2_feed_forward, a graph replay)
 * starts from the state the previous one left.  Runs on the engine stream, ordered with the forwards. */
void reset_rnn_state(network net, int b);

/* ---- text generation and scoring with [rnn] / [gru] networks (rnn.c) ----
 * The reference's entry points, and the y2_rnn_* calls they are written on.  The per-character loop runs on the device:
 * the sampled character becomes the next input row without leaving HBM, and the characters of one call are enqueued
 * with no host sync in between.  Tokens are step-major like the rows: [step][B], B = net.batch / time_steps sequences.
 * Refused with a message: a network without a recurrent layer, time_steps > 1 for generation, outputs < inputs, a seed
 * or text token outside [0, inputs) (a negative `char` included).  Strict mode, y2_set_graph and y2_set_timing work as
 * for network_predict. */
/* rnn.c:225: srand(rseed); the temperature on every layer; the first len-1 seed characters are predicted and printed,
 * the last one is the first generating input (an empty seed starts from token 0); num characters by the rule of
 * rnn.c:273-276 / sample_array (utils.c:520), printed "%c" or, with a token file, "%s ", then a newline.  The reference
 * draws its uniforms from a rand() stream that parse_network_cfg's weight initialisers (connected_layer.c) have
 * advanced; nothing is drawn at parse time here, so draw i uses the i-th value after srand(rseed). */
void test_char_rnn(char *cfgfile, char *weightfile, int num, char *seed, float temp, int rseed, char *token_file);
/* rnn.c:379: the seed is predicted, then the text on stdin is scored: per character the line of rnn.c:416 */
void valid_char_rnn(char *cfgfile, char *weightfile, char *seed);
/* rnn.c:420: per line on stdin: reset_rnn_state(net, 0), the seed, the line, a space; prints the line and ",%g" per value
 * of layer 0's output */
void vec_char_rnn(char *cfgfile, char *weightfile, char *seed);
char **read_tokens(char *filename, size_t *read);                /* rnn.c:39: one token per line */
/* srand(rseed), then u[i] = rand_uniform(0, 1) (utils.c:603-610: (float)rand() / RAND_MAX in float) for i < n: the
 * reference's generator (libc rand) and so its stream. */
int y2_rnn_uniforms(int rseed, int n, float *u);
/* Generate num characters on each of the B sequences, from the network's current state and temperature: the first
 * seed_len-1 rows of seed ([seed_len][B]) are predicted, the last is the first input (seed_len 0: token 0); draw i of
 * sequence b uses uniforms[i*B+b] and lands in tokens[i*B+b]; probs (or NULL) receives the row each draw sampled from,
 * [num][B][outputs].  n of the rule is the network's input size.  One sync, at the end; the state afterwards is the one
 * num-1+seed_len forwards leave, and a call seeded with the last row of tokens goes on where this one stopped. */
int y2_rnn_generate(network net, const int *seed, int seed_len, int num, const float *uniforms, int *tokens, float *probs);
/* Teacher-forced scoring of tokens ([n][B]): p_next[t*B+b] is the probability the network gave to tokens[t+1][b] after
 * reading tokens[0..t][b], for t < n-1; probs (or NULL) receives the rows, [n-1][B][outputs].  With time_steps T one
 * forward scores T characters per sequence; n-1 must be a multiple of T.  The state carries on across calls. */
int y2_rnn_score(network net, const int *tokens, int n, float *p_next, float *probs);
/* valid_char_rnn's books (rnn.c:402-416) over a text of n characters and the n-1 values y2_rnn_score gave for it: a float
 * sum of log(p)/(float)log(2), words counted on ' ', '\n', '\t' of the following character; the two values of :416
 * as floats (+inf where 2^(-sum/words) is beyond a float). */
int y2_rnn_perplexity(const float *p_next, const unsigned char *text, int n, float *perplexity, float *word_perplexity);
float *get_network_output_gpu(network net);                      /* network_kernels.cu:385 */
int get_network_output_size(network net);                        /* network.c:390 */
int get_network_input_size(network net);                         /* network.c:397 */
void top_predictions(network net, int k, int *index);            /* network.c:449 */
char *get_layer_string(LAYER_TYPE a);                            /* network.c:73 */

/* ---- region head hand-off (region_layer.h:12, box.h:13-17) ---- */
void get_region_boxes(layer l, int w, int h, float thresh, float **probs, box *boxes, int only_objectness, int *map);
void get_detection_boxes(layer l, int w, int h, float thresh, float **probs, box *boxes, int only_objectness);   /* detection_layer.c:222 (YOLOv1 head) */
void do_nms_sort(box *boxes, float **probs, int total, int classes, float thresh);   /* box.c:249 */
void do_nms(box *boxes, float **probs, int total, int classes, float thresh);        /* box.c:279 */
float box_iou(box a, box b);                                                         /* box.c:94  */
box float_to_box(float *f);                                                          /* box.c:5   */

/* ---- Kinect-pipeline entry (test_detector.h:2, detector.c:558) ---- */
void test_detector_img(char **names, image **alphabet, network net, image im, float thresh,
                       object *RecObects, int *objectNumPerFrame);
/* test_detector.h / detector.c:514-554: the detection runs on imFilter (the frame with everything but the graspable
 * objects whitened); `im` is only what the reference would draw on.  Objects are filled as test_detector_img fills them. */
void test_detector_img_for_grasping(char **names, image **alphabet, network net, image im, image imFilter, float thresh,
                                    object *RecObects, int *objectNumPerFrame);

/* ---- evaluation writers (detector.c:169-243) and the validate loops over in-memory frames ---- */
int get_coco_image_id(char *filename);                                                    /* detector.c:169 */
void print_cocos(FILE *fp, char *image_path, box *boxes, float **probs, int num_boxes, int classes, int w, int h);
void print_detector_detections(FILE **fps, char *id, box *boxes, float **probs, int total, int classes, int w, int h);
void print_imagenet_detections(FILE *fp, int id, box *boxes, float **probs, int total, int classes, int w, int h);
void print_yolo_detections(FILE **fps, char *id, box *boxes, float **probs, int total, int classes, int w, int h);   /* yolo.c:95 */
char *basecfg(char *cfgfile);                                                             /* utils.c:121 */
/* validate_detector (detector.c:245-368) with the image list replaced by `n` network-sized CHW frames in
 * memory: per frame network_predict -> get_region_boxes(l, orig_w, orig_h, .005, .., 0, map) ->
 * do_nms_sort(.45) -> the writer `eval` selects: "voc" (default; <prefix>/comp4_det_test_<name>.txt per
 * class, id = basecfg(path)), "coco" (<prefix>/coco_results.json), "imagenet" (200 classes,
 * <prefix>/imagenet-detection.txt).  A network ending in [detection] (YOLOv1) follows validate_yolo (yolo.c:116-200)
 * instead: get_detection_boxes at .001, do_nms_sort(.5), print_yolo_detections (voc files only).
 * Frames are processed net.batch at a time.  Returns 0 / -1. */
int y2_validate_detector_frames(network net, float *frames, int n, char **paths, int *orig_w, int *orig_h,
                                char *eval, char *prefix, char **names, int *map);
/* validate_detector_recall (detector.c:371-450): thresh .2, objectness-only decode, do_nms(.., 1, .4), IoU .5
 * against truth[truth_first[f] .. truth_first[f+1]) (relative centre-form boxes); prints the reference's
 * progress line per frame on stderr and returns the running totals. */
typedef struct { int total, correct, proposals; float avg_iou; } y2_recall;
int y2_validate_recall_frames(network net, float *frames, int n, const box *truth, const int *truth_first, y2_recall *res);
/* validate_classifier_single (classifier.c:469-529) over `n` network-sized CHW frames in memory: truth[f] is the class
 * the reference derives from the file path (-1 = none); per frame network_predict -> top_k -> running top-1 / top-k
 * accuracy, the reference's progress line on stdout; the final averages are returned.  Returns 0 / -1.
 * A hierarchical classifier ([softmax] tree=, net.hierarchy) follows classifier.c:514-520: hierarchy_predictions(pred,
 * outputs, hierarchy, 1) runs on the device before the rows come down.  The device applies the hierarchy of its own head
 * only: a net.hierarchy that is not the softmax_tree of the network's output [softmax] layer with n == outputs (a tree hung
 * on a flat classifier, a head with groups > 1) is refused before any device work, here and in every entry point below
 * that applies a hierarchy. */
int y2_validate_classifier_frames(network net, float *frames, int n, const int *truth, int classes, int topk,
                                  float *top1_out, float *topk_out);
/* The core of predict_classifier (classifier.c:716-718) over `n` network-sized CHW frames, net.batch at a time:
 * network_predict, with a hierarchy hierarchy_predictions(pred, outputs, hierarchy, 0) on the device, then top_k over all
 * net.outputs.  indexes[n][top], probs[n][top] (the values at those indexes).  A flat classifier has no hierarchy step.
 * Returns 0 / -1. */
int y2_classify_frames(network net, float *frames, int n, int top, int *indexes, float *probs);
/* hierarchy_predictions(row, outputs, net.hierarchy, only_leaves) (tree.c:37-51) on all net.batch rows of the output
 * layer's DEVICE copy, in place, on the engine's stream: for callers of y2_forward_device, before y2_output_enqueue /
 * y2_output_fetch.  The leaf flags are read from net.hierarchy->leaf at the call and sent up only when they changed since
 * the last call (change_leaves).  The rows are multiplied IN PLACE and nothing marks them as absolute: call it once per
 * forward -- a second call after the same forward (graph replay included), or a call after y2_classify_frames /
 * y2_validate_classifier_frames / a view mode, which have applied the hierarchy already, applies it twice.
 * Refused without net.hierarchy, and before the first forward.  Returns 0 / -1. */
int y2_hierarchy_enqueue(network net, int only_leaves);

/* ---- the reference's other three classifier evaluations, views built on the device (y2_tta.c) ----
 * Frames are `image` structs of any size in host memory (CHW float, at least net.c planes; the first net.c are read);
 * truth[f] as for y2_validate_classifier_frames.  Every view of a frame is predicted, the predictions are added into an
 * accumulator that starts at 0 (fp32, one rounding per addition, in the order given below -- axpy_cpu, classifier.c:393,
 * 577,580), and top_k is taken of the sum.  What a `mode` does per frame:
 *   Y2_VIEWS_CROP10  validate_classifier_10, classifier.c:373-395.  The frame is resized to (net.w+32) x (net.h+32) unless
 *       it has that size (load_image_color(path, w+shift, h+shift), image.c:2084).  Views, in this order: crop_image
 *       (image.c:1512-1532) to net.w x net.h at shifts (-32,-32) (32,-32) (0,0) (-32,32) (32,32), then the same five of
 *       the flip_image'd frame (image.c:1056-1070).  Two quirks are kept: (0,0) is the top-left window, not the centre,
 *       and the other four reach 32 pixels past an edge, where crop_image's constrain_int repeats the edge pixel.
 *   Y2_VIEWS_MULTI   validate_classifier_multi, classifier.c:572-582.  Per scale s, in the order given: (rw, rh) =
 *       resize_min's dimensions (image.c:1662-1672: w < h ? (s, h*s/w) : (w*s/h, s), integers); the frame is resized to
 *       them (not at all when equal, image.c:1673), the network is resized to (rw, rh), the whole image is predicted, then
 *       its mirror image.  scales == NULL: the reference's 224, 288, 320, 352, 384 (classifier.c:550).
 *   Y2_VIEWS_FULL    validate_classifier_full, classifier.c:436-452.  One scale, net.w as it was on entry; one unflipped
 *       view of the whole resized image.
 * A hierarchical classifier (net.hierarchy: the tree of the output [softmax] tree= layer) gets hierarchy_predictions(pred,
 * outputs, hierarchy, 1) on a view's prediction before it is added, on the device (a row mask per forward, no copy and no
 * wait): all ten views of CROP10 (classifier.c:392), FULL's one (:453), but of MULTI only the UNFLIPPED views (:576) -- the
 * reference adds the flipped view's prediction as network_predict returned it, conditional probabilities and all
 * (:579-580).  That quirk is kept.  The head's tree tables are derived again by every plan but sent up only when they differ
 * from what the device holds, so the re-plans of MULTI / FULL cost a hierarchical network no copy and no wait either: per
 * block it resizes, copies down and waits exactly as often as a flat classifier of the same shape.
 * How it runs: a block of consecutive frames goes up in ONE copy; the resizes, the views (one launch per forward), the
 * forwards of net.batch views -- packed image-major, an image's views may straddle two forwards, unused slots are zero --
 * and one accumulation launch per forward are enqueued on the engine's stream; the host syncs once per block and the
 * block's sums come down in ONE copy.  MULTI and FULL go size-major inside a block: per scale the frames whose resized
 * size is equal are grouped and the network is resized once per distinct size (y2_view_resizes counts these), not once
 * per frame and scale; every accumulator still receives its rows in the order above, so the sums equal the image-major
 * loop's bit for bit.  A block holds its sources, the largest scale's resized copies and its accumulators in at most
 * Y2_VIEW_BLOCK_BYTES of HBM (one frame always goes); y2_set_view_block_bytes (0 = the default) or env
 * Y2_VIEW_BLOCK_BYTES override it.  On return the network has the size and batch it had on entry; its plan is rebuilt at
 * the next predict, as after any resize_network (hence the network * signatures).
 * Refused before any device work, with a message naming the argument or the frame: n <= 0; NULL frames, sums or truth;
 * a frame without data, with w or h <= 0 or with fewer than net.c planes; classes > outputs; topk > classes; nscales <= 0
 * with a scale list; a scale <= 0; a net.hierarchy that is not the output head's tree (above); a recurrent network; for MULTI / FULL a
 * network resize_network refuses (the layer is named: [connected] in alexnet.cfg) or a frame too small for it at some
 * scale.  Strict mode, fp16 mode and y2_set_graph work as for network_predict. */
enum { Y2_VIEWS_CROP10 = 0, Y2_VIEWS_MULTI = 1, Y2_VIEWS_FULL = 2 };
#define Y2_VIEW_BLOCK_BYTES ((size_t)256 << 20)
void y2_set_view_block_bytes(size_t bytes);
unsigned long y2_view_resizes(void);             /* resize_network calls the view modes made for their size groups */
/* sums: n x outputs, the summed predictions of each frame */
int y2_classifier_view_sums(network *net, int mode, const image *frames, int n, const int *scales, int nscales, float *sums);
/* The reference's loops around it: top_k of each sum, the running top-1 / top-k accuracy, the progress line
 * "%d: top 1: %f, top %d: %f\n" per frame on stdout in frame order; the final averages are returned.  0 / -1. */
int y2_validate_classifier_10_frames(network net, const image *frames, int n, const int *truth, int classes, int topk,
                                     float *top1, float *topk_out);
int y2_validate_classifier_multi_frames(network *net, const image *frames, int n, const int *scales, int nscales,
                                        const int *truth, int classes, int topk, float *top1, float *topk_out);
int y2_validate_classifier_full_frames(network *net, const image *frames, int n, const int *truth, int classes, int topk,
                                       float *top1, float *topk_out);

/* ---- small helpers the callers use (option_list.h:12-19, data.c:474, utils.c, tree.c, image.c) ---- */
list *read_data_cfg(char *filename);
char *option_find(list *l, char *key);
char *option_find_str(list *l, char *key, char *def);
int option_find_int(list *l, char *key, int def);
int option_find_int_quiet(list *l, char *key, int def);
float option_find_float(list *l, char *key, float def);
float option_find_float_quiet(list *l, char *key, float def);
void free_list(list *l);
char **get_labels(char *filename);
image **load_alphabet(void);               /* glyph PNGs are UI (image.c:212): returns NULL here */
tree *read_tree(char *filename);           /* tree.c:53 */
void change_leaves(tree *t, char *leaf_list);   /* tree.c:7: leaf[i] = t->name[i] is a line of the file; "Found %d leaves." on stderr */
float get_hierarchy_probability(float *x, tree *hier, int c);   /* tree.c:27: x[c] times x of every ancestor */
void hierarchy_predictions(float *predictions, int n, tree *hier, int only_leaves);   /* tree.c:37: on the host, in place */
int *read_map(char *filename);             /* utils.c:17 */
int max_index(float *a, int n);            /* utils.c:533 */
void top_k(float *a, int n, int k, int *index);   /* utils.c:179 */
void mean_arrays(float **a, int n, int els, float *avg);   /* utils.c:420 */
image make_image(int w, int h, int c);     /* image.c:1436 */
void free_image(image m);                  /* image.c:2245 */
image resize_image(image im, int w, int h);/* image.c:1950; runs on the GPU */
image letterbox_image(image im, int w, int h);                   /* image.c:1624; runs on the GPU */
void letterbox_image_into(image im, int w, int h, image boxed);  /* image.c:1607; runs on the GPU */
float get_color(int c, int x, int max);    /* image.c:33 */
void error(const char *s);                 /* utils.c:195: perror + exit(-1) */
void file_error(char *s);                  /* utils.c:208: message + exit(0) */

/* ------------------------------------------------------------------------- */
/* Extensions (not in the reference): batched, HBM-resident operation        */
/* ------------------------------------------------------------------------- */

/* one detection of y2_detect*: centre-form box scaled by (img_w,img_h) of the call */
typedef struct { float x, y, w, h, prob; int obj_id; } y2_det;

/* Build plan, allocate HBM and upload weights now instead of at the first predict.  Returns 0 or <0. */
int y2_prepare(network *net);
/* Force every convolution through the reference-order VALU kernel (bit-identical to the CPU path). */
void y2_set_strict(network *net, int strict);
/* conv -> 2x2/2 maxpool pairs are fused by default (the conv pools in its epilogue and the
 * full-resolution activation is never stored); 0 turns that off, e.g. to inspect every layer. */
void y2_set_fusion(network *net, int on);
/* Measure instead of model: when the plan is (re)built, every convolution that runs on the fp32 matrix cores times
 * each instantiated tile shape (and a few K-splits) inside whole forward passes and keeps the fastest (y2h_conv_candidates); the result
 * is remembered per layer shape for the life of the process.  Costs about a second per network at plan time.  A tile
 * shape never changes a result bit; a different K-split changes the last bits of that layer (fixed-order partial sums).
 * Off by default; env Y2_AUTOTUNE=1 turns it on for every network.  Ignored in strict mode. */
void y2_set_autotune(network *net, int on);
/* Throughput mode for callers that pipeline batches with y2_detect_enqueue / y2_detect_fetch: decode, NMS and
 * compaction of batch i run on a stream of their own, so their small grids (one workgroup per image and class group)
 * share the GPU with the forward pass of batch i+1 instead of idling it; the forward pass waits for them only before
 * its region layer overwrites the tensor they read.  Results are identical.  Off by default (a lone
 * y2_detect_resident call gains nothing and pays two more events); region heads only. */
void y2_set_detect_overlap(network *net, int on);
/* Record the forward pass's kernel launches into a hipGraph at the next call and replay it afterwards (one
 * hipGraphLaunch instead of 20-60 launches; for batch-1 callers such as test_detector_img).  The graph is tied to
 * the plan and to the input pointer: a resize / set_batch / mode switch or a different device input re-records.
 * Off by default; env Y2_GRAPH=1 turns it on for every network.  Ignored in strict mode and while layer timing is on. */
void y2_set_graph(network *net, int on);
/* The packed, kernel-layout weight arena (one allocation; what a multi-GPU launcher broadcasts). */
int y2_weights_arena(network *net, void **dev_ptr, size_t *bytes);
/* fp16 storage mode (no reference counterpart; BASELINE configs[4]): activations and packed weights are
 * IEEE half in HBM, convolutions accumulate in fp32 on the fp16 matrix cores, batch-norm is folded into one
 * fp32 fma, the region / avgpool / softmax heads stay fp32.  Takes effect at the next forward (the plan is
 * rebuilt).  Ignored while strict mode is on.  Env Y2_FP16=1 turns it on for every network. */
void y2_set_half(network *net, int on);
/* Declare the arena contents valid although load_weights was not called on this process
 * (e.g. it was filled by an RCCL broadcast from rank 0). */
void y2_weights_resident(network *net);
/* Multi-GPU (one process per GPU, frames sharded): replicate root's packed weights with ONE in-place RCCL broadcast of
 * the arena over xGMI -- replaces the host-staged distribute_weights of network_kernels.cu:240-250.  `comm` is an
 * ncclComm_t of the RCCL this process uses (y2_comm_library() names it); the three y2_comm_* helpers create one
 * without any other dependency: rank 0 calls y2_comm_unique_id and hands the 128 bytes to the other ranks by whatever
 * channel the launcher has (a file, a socket, an env variable), then every rank calls y2_comm_init_rank.  Root must
 * have called load_weights; the other ranks only parse the cfg.  Returns 0 or <0 (y2_last_error()). */
#define Y2_COMM_ID_BYTES 128
const char *y2_comm_library(void);
int y2_comm_unique_id(void *id_out);
int y2_comm_init_rank(void **comm, int nranks, const void *id, int rank, int device);
int y2_comm_destroy(void *comm);
int y2_broadcast_weights(network *net, void *comm, int root);
/* ranks of `comm` and this process's rank in it, as RCCL reports them (ncclCommCount / ncclCommUserRank) */
int y2_comm_count(void *comm, int *nranks, int *rank);
/* (layout signature, bytes) of the weight arena under the current plan.  y2_broadcast_weights compares them across the
 * ranks before it moves a byte (RCCL itself checks neither counts nor types); a launcher that replicates the arena by
 * other means must do the same. */
int y2_weights_layout(network *net, unsigned long long *signature, size_t *bytes);
/* C face of the C++ Detector class (include/yolo_v2_class.hpp) for FFI callers that cannot bind a C++ class (ctypes, cgo,
 * JNI).  y2_detector_detect = Detector::detect(image_t) [+ Detector::tracking when track != 0]: `chw` is a planar float
 * image in [0,1], up to `max` results are written to `out` in bbox_t's own layout (4 unsigned, float, 2 unsigned = 28
 * bytes each); returns the number of boxes (may exceed max) or < 0 with the message in y2_last_error().  nms < 0 keeps
 * the detector's current Detector::nms. */
void *y2_detector_create(const char *cfg, const char *weights, int gpu_id);
void  y2_detector_destroy(void *det);
int   y2_detector_net_size(void *det, int *w, int *h);
int   y2_detector_detect(void *det, const float *chw, int c, int h, int w, float thresh, int use_mean, float nms, int track,
                         void *out, int max);
/* Pinned, multi-buffered host feed (replaces the per-call cudaMalloc + pageable H2D + cudaFree of
 * network_kernels.cu:392-405): `slots` pairs of (pinned host buffer, HBM buffer) of slot_bytes each (0 = one batch of
 * float NCHW frames) and a copy stream.  The producer writes a batch into y2_feed_host(net, s), y2_feed_submit starts
 * its upload, y2_feed_forward / y2_feed_forward_u8 (camera frames [batch][h][step] bytes, as y2_ingest_u8) make the
 * forward wait ON THE DEVICE for that upload -- so batch i+1 crosses PCIe while batch i computes.  Follow with
 * y2_detect_enqueue / y2_detect_fetch.  y2_feed_wait_host blocks until a slot's pinned buffer may be overwritten. */
int y2_feed_open(network *net, int slots, size_t slot_bytes);
void y2_feed_close(network *net);
void *y2_feed_host(network net, int slot);
void *y2_feed_device(network net, int slot);
size_t y2_feed_slot_bytes(network net);
int y2_feed_submit(network net, int slot, size_t bytes);
int y2_feed_wait_host(network net, int slot);
int y2_feed_forward(network net, int slot);
int y2_feed_forward_u8(network net, int slot, int h, int w, int c, int step, int swap_rb, int letterbox);
/* network_predict with the input already in HBM (NCHW, batch*inputs floats).  The returned
 * pointer is the same host buffer network_predict returns. */
float *y2_network_predict_device(network net, const float *d_input);
/* The host copy of the output as two halves, for callers that keep the device busy across batches (classifiers):
 * y2_forward_device(i); y2_output_enqueue(); y2_forward_device(i+1); p = y2_output_fetch();  -- the fetch waits for
 * batch i's copy only and returns the same host buffer network_predict returns (valid until the next enqueue). */
int y2_output_enqueue(network net);
float *y2_output_fetch(network net);
/* Forward only (no host copy of the output); then decode+NMS+collect with y2_detect_resident. */
int y2_forward_device(network net, const float *d_input);
/* Decode + per-class NMS + compaction of the last forward, all on device; up to max_per_image
 * detections per image are written to dets[b*max_per_image ...], counts[b] = number found. */
int y2_detect_resident(network net, float thresh, float nms, int img_w, int img_h,
                       y2_det *dets, int *counts, int max_per_image);
/* Its two halves, for callers that keep the device busy across batches: y2_detect_enqueue(i); y2_forward_device(i+1);
 * y2_detect_fetch(i) -- the fetch waits for batch i's results only (an event behind their D2H copies), so the host-side
 * wait and unpacking overlap the next forward pass.  One enqueue may be outstanding per network. */
int y2_detect_enqueue(network net, float thresh, float nms, int img_w, int img_h);
int y2_detect_fetch(network net, y2_det *dets, int *counts, int max_per_image);
/* Same on the average of the last three forwards' region outputs (Detector::detect use_mean, yolo_v2_class.cpp:
 * 208-213): the three-slot ring and the average live in HBM; slots start zeroed like the reference's calloc. */
int y2_detect_mean(network net, float thresh, float nms, int img_w, int img_h,
                   y2_det *dets, int *counts, int max_per_image);
/* Host-input convenience: H2D + forward + y2_detect_resident. */
int y2_detect(network net, float *input, float thresh, float nms, int img_w, int img_h,
              y2_det *dets, int *counts, int max_per_image);
/* Camera-frame entry: `batch` 8-bit interleaved frames (h x w x c, row pitch `step` bytes; swap_rb
 * exchanges channels 0 and 2 = BGR->RGB) are uploaded as bytes, converted to [0,1] planes, resized
 * (letterbox != 0: letterboxed) to the network input on the device, then forward + y2_detect_resident.
 * Same result as ipl_to_image + rgbgr_image + resize_image/letterbox_image + the float path
 * (yolo_v2_class.hpp:94-141, yolo_v2_class.cpp:173-249).  y2_ingest_u8 stops after filling the
 * network's device input (follow with y2_forward_device(net, NULL)). */
/* Float CHW frame of any size (batch-1 networks): its first net.c planes go up and are resized on the device
 * straight into the network input -- resize_image + the input copy of network_predict (detector.c:567-573)
 * without a host round trip.  Follow with y2_forward_device(net, NULL) / y2_network_predict_device(net, NULL). */
int y2_ingest_image(network net, image im);
int y2_ingest_u8(network net, const unsigned char *frames, int h, int w, int c, int step, int swap_rb, int letterbox);
int y2_detect_u8(network net, const unsigned char *frames, int h, int w, int c, int step, int swap_rb, int letterbox,
                 float thresh, float nms, int img_w, int img_h, y2_det *dets, int *counts, int max_per_image);
/* Regions of frames of any size in one forward pass (the Kinect loop's whole frame + two hand crops,
 * KinectUtil_with_cam.cpp:1029-1110, as one batch).  One region of an 8-bit interleaved frame in host memory
 * (h x w x c, row pitch `step` bytes); rw = rh = 0 means the whole frame (then x and y must be 0).
 * Item i becomes batch slot i: only its rows are packed, with a small descriptor table, into one pinned staging
 * buffer that goes up in ONE H2D copy, and one kernel (y2h_regions_to_input) fills the whole network input -- bit
 * for bit what y2_ingest_u8 computes for the copied crop (u8 -> planes, swap_rb, resize or letterbox).  Slots
 * n .. net.batch-1 are zeroed; the full planned batch still runs.  Every argument is checked before any device
 * work: n outside [1, net.batch], a NULL data pointer, step < w*c, c < net.c, a region outside its frame or a
 * degenerate letterbox is refused with a message naming the item, and nothing is uploaded or launched. */
typedef struct { const unsigned char *data; int h, w, c, step; int x, y, rw, rh; } y2_region;
int y2_ingest_regions(network net, const y2_region *items, int n, int swap_rb, int letterbox);
/* y2_ingest_regions + y2_forward_device + decode / NMS / compaction (y2_detect_resident with img_w = img_h = 1).
 * counts[0..n-1] and dets[i*max_per_item ..] are written for the n items only; boxes are relative to each item's
 * FRAME (y2_region_box_to_frame). */
int y2_detect_regions(network net, const y2_region *items, int n, int swap_rb, int letterbox,
                      float thresh, float nms, y2_det *dets, int *counts, int max_per_item);
/* A box relative to the network input -> relative to the item's frame (W x H), in place, fp32 in this order:
 *   letterbox:  (nw, nh) = y2h_letterbox_dims(rw, rh, net_w, net_h);
 *               x = (x*net_w - (net_w-nw)/2) / nw,  w = w*net_w / nw,  the same for y, h  ((..)/2 is integer)
 *   region:     x = (x*rw + rx) / W,  y = (y*rh + ry) / H,  w = w*rw / W,  h = h*rh / H   (KinectUtil_with_cam.cpp:1033-1036)
 * A whole-frame item skips the region step (it is the identity), so without a letterbox its boxes are returned
 * unchanged -- exactly what y2_detect_u8 returns for that frame. */
void y2_region_box_to_frame(const y2_region *item, int net_w, int net_h, int letterbox, float *x, float *y, float *w, float *h);
/* test_detector_img (detector.c:558) over n regions in one pass: BGR frames as the application's cv::Mat holds them
 * (swap_rb), resized (no letterbox), nms .1, objects filled exactly as test_detector_img fills them -- appended at
 * RecObjects[i][objectNumPerRegion[i]], which is incremented -- with boxes relative to each item's frame.
 * RecObjects[i] holds room for l.w*l.h*l.n objects.  net.batch >= n (set_batch_network). */
void test_detector_regions(char **names, network net, const y2_region *items, int n, float thresh,
                           object **RecObjects, int *objectNumPerRegion);
/* ------------------------------------------------------------------------- */
/* The depth stage of the Kinect RGB-D loop, on the device behind the detect  */
/* chain (KinectUtil_with_cam.cpp:394-442 drawDepth, :1866-1888                */
/* colorImgFilterbyDistance, :1482-1562 caculateXYZinCameraSpace, :1632-1706   */
/* objectBelong2Person).  All sums are integer sums (depth in 64 bits: the     */
/* reference's `int` overflows on a full-frame box at ordinary ranges, which   */
/* is not reproduced); the float steps are single IEEE operations.             */
/* ------------------------------------------------------------------------- */
typedef struct {
    const uint16_t *depth;   /* dh x dw, millimetres */
    const uint8_t  *body;    /* dh x dw, 1..6 = a tracked person, anything else none; NULL = no bodies */
    const float    *map;     /* H x W x 2: (X, Y) in the depth frame for every colour pixel (MapColorFrameToDepthSpace);
                                NULL = already registered: needs H == dh, W == dw, identity */
    int dh, dw, H, W;
} y2_depth_frame;
/* One H2D copy (pinned staging, grow-only) + the alignment kernel, on the engine's stream.  Per colour pixel (:407-423):
 * dx = (int)(X + 0.5f), dy likewise (truncation toward zero: X = -0.7 lands on column 0); inside [0,dw) x [0,dh):
 * depth16 = depth, depth8 = (uint8_t)(depth >> 5), person = body (255 without a body frame); otherwise 0, 0, 255.  A
 * coordinate that is not finite or outside int range is unmapped.  The planes stay in HBM until the next upload.
 * dh, dw <= 32767. */
int y2_depth_upload(network net, const y2_depth_frame *f);
/* GetDepthFrameToCameraSpaceTable: dh x dw x 2 floats, sent once.  The SDK's MapDepthPointToCameraSpace is closed; this
 * library DEFINES a depth-space point (px, py) at z metres to map to (tab[iy][ix].x * z, tab[iy][ix].y * z, z) with
 * ix = (int)(px + 0.5f), iy likewise, and to (-inf, -inf, -inf) outside the table.  Without a table the camera fields
 * of y2_det3d are (0, 0, -1, 0, 0).  tab == NULL drops the table. */
int y2_depth_set_camera_table(network net, const float *tab, int dh, int dw);
/* Fetch the aligned planes (H x W each; any pointer may be NULL). */
int y2_depth_aligned(network net, uint16_t *depth16, uint8_t *depth8, uint8_t *person);

/* Per-box result.  ROI (:1501-1504, y2_depth_roi); otsu = otsuThreshold of depth8 in the ROI (y2_otsu_threshold);
 * mean_all_mm = sum(depth16) / n (KinectUtil.cpp:489-501); avg_mm = GetImgAvg(depth16, otsu * 32) - 16 (:1526, integer
 * division); owner = the body label 1..6 with the most pixels (a tie goes to the lower label; the reference's answer
 * depends on which label it meets first), belongs = (float)count / n > 0.5, body_id = that label or 255 (:1684-1703);
 * pts = centre, top, bottom, left, right depth-space points of caculateXY (:1366-1452; the centre test compares depth8
 * with otsu * 32 as the reference does); cam_* = :1540-1559 through the camera table.  An empty ROI (the reference
 * would hit an OpenCV assertion) gives valid = 0, zeros and cam_z = -1. */
typedef struct { int valid, left, top, right, bot, otsu, mean_all_mm; float avg_mm; int body_id, belongs;
                 float cam_x, cam_y, cam_z, cam_w, cam_h; float pts[5][2]; } y2_det3d;
/* otsuThreshold (:1564-1630) of a 256-bin histogram, the very code the kernel runs (include/y2_depth_rule.h). */
int y2_otsu_threshold(const int hist[256]);
/* The ROI of a frame-relative box in a W x H frame; returns 1 when it is not empty. */
int y2_depth_roi(box b, int W, int H, int *left, int *top, int *right, int *bot);
/* Statistics of n caller-given frame-relative boxes against the uploaded planes. */
int y2_depth_boxes(network net, const box *boxes, int n, y2_det3d *out);
/* y2_ingest_regions with the hand-crop distance filter fused into the source read: item i with far_m[i] > 0 (the caller
 * passes jointDistance + 0.3) reads a source pixel at frame position (r, c) as 255 in every plane when
 * depth8[r][c] <= 15 || (float)depth8[r][c] >= far_m * 1000 / 32 (fp32, that order, :1879).  far_m[i] <= 0: no filter;
 * with every far_m <= 0 the input is bit-identical to y2_ingest_regions.  Refused before any device work, besides what
 * y2_ingest_regions refuses: a filtered item with fewer than 3 channels, no uploaded depth frame, a filtered item whose
 * frame is not the uploaded H x W. */
int y2_ingest_regions_depth(network net, const y2_region *items, int n, const float *far_m, int swap_rb, int letterbox);
/* y2_detect_regions with that ingest (far_m == NULL: no filter), and behind the detect chain, on the same stream with no
 * host synchronisation in between, the statistics of every kept detection (its box mapped into its frame on the
 * device): d3[i*max_per_item + j] belongs to dets[i*max_per_item + j].  Needs an uploaded depth frame. */
int y2_detect_regions_depth(network net, const y2_region *items, int n, const float *far_m, int swap_rb, int letterbox,
                            float thresh, float nms, y2_det *dets, y2_det3d *d3, int *counts, int max_per_item);
/* test_detector_regions + the eight depth fields of `object`: CameraX/Y/Z, CameraWidth, CameraHeight,
 * flagBelong2Person, bodyId (far_m == NULL: no filter). */
void test_detector_regions_depth(char **names, network net, const y2_region *items, int n, const float *far_m, float thresh,
                                 object **RecObjects, int *objectNumPerRegion);
/* ------------------------------------------------------------------------- */
/* The Grasp branch of the Kinect loop: the table plane removed on the device  */
/* behind y2_depth_upload (KinectUtil_with_cam.cpp:364-377 updateDepth ->      */
/* :1931-1974 desk_seg -> plane_seg.cpp:157-213).  PCL's sampler is seeded from */
/* the clock and the SDK's camera mapping is closed, so this library DEFINES a */
/* deterministic RANSAC: include/y2_plane_rule.h is its one statement, compiled */
/* by the host and the kernels alike.  All hypotheses are evaluated (no         */
/* adaptive early stop).                                                        */
/* ------------------------------------------------------------------------- */
/* far_m: depth beyond it is clipped to 0 (:1944-1950); dist_m: the inlier distance; iters: hypotheses (<= 256); seed: the
 * sampler's start state, restarted at every upload; samples: NULL, or iters triples of depth-pixel indices to use instead
 * of the sampler (copied).  The reference's values are 1.0, 0.02, 50. */
typedef struct { float far_m, dist_m; int iters; unsigned seed; const int *samples; } y2_plane_opts;
/* NULL or iters <= 0 turns the removal off, which is the default: y2_depth_upload then enqueues what it always did.
 * Refused: iters > 256, far_m or dist_m not finite or <= 0.  Takes effect at the next y2_depth_upload, which with the
 * removal on refuses, before any copy, a missing camera table or one whose size is not the depth frame's. */
int y2_depth_set_plane_removal(network net, const y2_plane_opts *o);
/* found = 0: no plane (fewer than 3 valid points, every hypothesis void, or a best count below 3); then best = -1,
 * best_count = 0, the coefficients are 0 and nothing is removed.  best: the winning hypothesis (largest inlier count, a
 * tie to the lowest index); valid_points: pixels with 0 < depth <= far_m; removed: valid pixels within dist_m of the
 * refitted plane a*x + b*y + c*z + d = 0 (unit normal, d >= 0: oriented towards the camera). */
typedef struct { int found, best, valid_points, best_count, removed; double a, b, c, d; } y2_plane;
int y2_depth_plane(network net, y2_plane *out);
/* grasp_depth (dh x dw): the clipped depth with the plane's pixels zeroed (depthBufferGrasping); grasp16 (H x W): that
 * registered to the colour frame (i_RgbTodepthForGrasping, :402-438), 0 where unmapped.  Either pointer may be NULL. */
int y2_depth_grasp_aligned(network net, uint16_t *grasp_depth, uint16_t *grasp16);
/* Which branch of caculateXYZinCameraSpace (:1508-1527) y2_depth_boxes, y2_detect_regions_depth,
 * test_detector_regions_depth and Detector::detect_regions_depth compute.  GRASP: avg_mm = GetImgAvg(grasp16 ROI, 255*32)
 * with nothing subtracted, otsu reported as 255 (so the centre point takes every mapped pixel); every other field as in
 * DEMO_WHAT, the default.  GRASP on a frame uploaded without plane removal is refused when the statistics are asked for. */
enum { Y2_EVENT_DEMO_WHAT = 0, Y2_EVENT_GRASP = 1 };
int y2_depth_set_event(network net, int event);
/* on: a filtered item (far_m[i] > 0) of the *_depth ingests also reads a source pixel as 255 in every plane where grasp16
 * is 0 -- the imFilter of test_detector_img_for_grasping, formed on the device.  Off (the default): the ingest is
 * bit-identical to what it was. */
int y2_depth_set_grasp_filter(network net, int on);
/* The rule itself, host-callable: the very code the kernels run (include/y2_plane_rule.h).
 * y2_plane_samples: the sampler over a depth frame -> iters triples of depth-pixel indices ((-1,-1,-1) = void); returns the
 *   number of filled triples, -1 on bad arguments.
 * y2_plane_from_points: the fp32 plane (nx, ny, nz, d) through three points; 0 = degenerate.
 * y2_plane_fit: the refit from the ten sums n, x, y, z, xx, xy, xz, yy, yz, zz -> (a, b, c, d); 0 = no plane. */
int y2_plane_samples(const uint16_t *depth, int dh, int dw, float far_m, int iters, unsigned seed, int *triples);
int y2_plane_from_points(const float *p0, const float *p1, const float *p2, float *plane);
int y2_plane_fit(const double *sums, double *plane);
/* ------------------------------------------------------------------------- */
/* The KCF trackers of the Kinect loop, on the device, all objects in one      */
/* batch (KinectUtil_with_cam.cpp:764-803 InitialTracker / test_tracker_img    */
/* over kcf.cpp, complexmat.hpp, piotr_fhog/), with the fork's parameters      */
/* (kcf.h:51-57: padding 3.0, kernel sigma 0.5, lambda 1e-4, interpolation     */
/* 0.02, output sigma factor 0.1, cell 4).  No scale adaptation, as in the     */
/* reference.  OpenCV's cvtColor, resize and dft are not linked; this library  */
/* DEFINES: grey = (1868*B + 9617*G + 4899*R + 8192) >> 14 of an 8-bit BGR /   */
/* BGRA pixel (a 1-channel frame is taken as is); the halving of a frame as    */
/* round-half-even(0.5*cols) x round-half-even(0.5*rows) pixels with taps      */
/* (-3, 19, 19, -3)/32 at source columns 2d-1 .. 2d+2 clamped to the image,    */
/* horizontal pass first, then vertical, in fp32; the DFT as a dense product   */
/* with twiddles of (j*k) mod n.  Parity with OpenCV is unpinned.              */
/* ------------------------------------------------------------------------- */
#define Y2_KCF_MAX_TRACKERS 32
/* A feature map has at most 256 cells per side: a window of 1024 px, a box of 256 px per side in the tracker's own scale.
 * A box with w*h > 10000 is tracked at half resolution, so that is a box of roughly 512 px on a side in the frame. */
#define Y2_KCF_MAX_CELLS 256
typedef struct { double cx, cy, w, h; } y2_kcf_box;            /* BBox_c, pixels of the frame */
typedef struct { int resized, win_w, win_h, cells_w, cells_h; double cx, cy, w, h, output_sigma; } y2_kcf_geometry;
/* init's arithmetic (kcf.cpp:7-27), device-free: the halving rule (w*h > 100.*100. strictly), the pose in the tracker's
 * scale, the window floor(w * 4) x floor(h * 4), its cells (window / 4) and p_output_sigma.  Refused (-1): a box that is
 * not finite or has w <= 0 or h <= 0, a feature map above Y2_KCF_MAX_CELLS per side or below 2 x 2 cells. */
int  y2_kcf_plan(const y2_kcf_box *b, y2_kcf_geometry *g);
/* KCF_Tracker::init of n trackers on one frame (h x w x c bytes, c = 1, 3: BGR, 4: BGRA, rows `step` bytes apart); the
 * trackers of an earlier init are dropped.  Only the frame rows the windows touch are uploaded, in one copy.  Refused by
 * name before any device work: n < 1 or n > Y2_KCF_MAX_TRACKERS, a NULL frame or box list, c other than 1, 3, 4,
 * step < w*c, and what y2_kcf_plan refuses. */
int  y2_kcf_init(network net, const unsigned char *frame, int h, int w, int c, int step, const y2_kcf_box *boxes, int n);
/* KCF_Tracker::track of every tracker on a new frame -> out[i] = getBBox(), peak[i] = the response maximum (either may be
 * NULL).  update = 0: what the application's copy-and-drop call gives (the stored model and pose stay as they are, the
 * retraining half is skipped); update != 0: the stored tracker is retrained and moves.  Refused before any device work:
 * no trackers (y2_kcf_init first), a frame whose size or channel count differs from the init frame's, a NULL frame,
 * step < w*c. */
int  y2_kcf_track(network net, const unsigned char *frame, int h, int w, int c, int step, int update, y2_kcf_box *out, float *peak);
int  y2_kcf_count(network net);
/* The tests' window: tensor `what` of tracker i as of the last call.  PATCH: win_h x win_w grey; FEATURES: 31 x R x C
 * (no window); XF: the model, 31 x 2 x R x C (real plane, imaginary plane); ALPHAF: 2 x R x C; RESPONSE: R x C of the
 * last track.  `floats` must be the tensor's size. */
enum { Y2_KCF_PATCH = 0, Y2_KCF_FEATURES = 1, Y2_KCF_XF = 2, Y2_KCF_ALPHAF = 3, Y2_KCF_RESPONSE = 4 };
int  y2_kcf_fetch(network net, int i, int what, float *dst, size_t floats);
/* The DFT kernels alone: forward, src real rows x cols -> dst 2 x rows x cols; inverse, src 2 x rows x cols -> dst the
 * real part, rows x cols, scaled by 1/(rows*cols).  2 <= rows, cols <= Y2_KCF_MAX_CELLS.  Leaves the trackers alone. */
int  y2_kcf_dft(network net, const float *src, int rows, int cols, int inverse, float *dst);
void y2_kcf_free(network net);
/* the application's two calls, objects relative to the frame as it holds them (KinectUtil_with_cam.cpp:764-803):
 * InitialTracker (bb = x*W, y*H, w*W, h*H in fp32; the objects are kept as tracking_objects) and test_tracker_img
 * (update = 0; objs[i] = tracking_objects[i] with x, y, w, h = cx/W, cy/H, w/W, h/H; *n = the tracker count). */
void y2_kcf_init_objects(network net, const unsigned char *frame, int h, int w, int c, int step, const object *objs, int n);
void y2_kcf_track_objects(network net, const unsigned char *frame, int h, int w, int c, int step, object *objs, int *n);
/* ------------------------------------------------------------------------- */
/* Training on the device: the other half of network.c (train_network_datum     */
/* :225-243 = forward with train = 1, backward_network, update_network), fp32   */
/* (the convolution products optionally on the bf16 matrix cores, see           */
/* y2_train_set_precision),                                                     */
/* for convolutional classifiers, YOLOv2 detectors ([region] loss, [route],     */
/* [reorg]; the truth of a [region] network is [batch][150]) and YOLOv1          */
/* detectors ([connected], [dropout], [detection] loss; the truth is            */
/* [batch][side*side*(1+coords+classes)], the load_data_region layout; see      */
/* y2_train_truth_floats).  The trainer owns its buffers (master                */
/* weights, update buffers, per layer output / delta / x / x_norm / mean /      */
/* variance); the inference plan is untouched, struct network and struct layer  */
/* keep their layout and layer.delta stays NULL.                                */
/* Trainable: [convolutional] (any size / pad, stride 1, batch_normalize 0 / 1, */
/* linear / leaky / logistic / relu), [maxpool], [avgpool], [softmax] (groups   */
/* 1, no tree), [cost] type=sse; in a network that ends in [region] also        */
/* [route], [reorg] (reverse=0) and the [region] head (softmax=1, no tree= /    */
/* map=, classfix=0); in a network that ends in [detection] also [connected]    */
/* (batch_normalize 0 / 1, the same four activations; its products are fp32 in  */
/* every precision mode), [dropout] (its draws are libc rand() in the           */
/* reference's order: srand() before a step fixes them) and the [detection]     */
/* head (coords=4, random=0, last layer).  Refused by name before any device allocation,            */
/* layer number and type in y2_last_error(): every other section type, stride   */
/* > 1, xnor, another activation, adam=1, policy=random, another cost type, a   */
/* tree / groups > 1 softmax, fp16 mode, a recurrent network, a batch-normalised */
/* layer with batch * out_h * out_w < 2 (the reference divides by zero).        */
/* Every reduction has a fixed order: a step run twice from the same state      */
/* gives the same bytes.                                                        */
/* ------------------------------------------------------------------------- */
/* network.c:225: *net.seen += net.batch; forward(train); backward; the loss; the update when
 * (*net.seen / net.batch) % net.subdivisions == 0.  x: [batch][c][h][w], y: [batch][outputs], host memory.  Prepares
 * lazily.  Returns the loss (get_network_cost), NAN after a failure. */
float train_network_datum(network net, float *x, float *y);
float get_current_rate(network net);             /* network.c:48: constant, step, steps, exp, poly (burn_in), sig */
int get_current_batch(network net);              /* network.c:31 */
float get_network_cost(network net);             /* network.c:183: mean of the [cost] layers' cost[0] */
/* Builds the trainer from the host weights (load_weights, or whatever the layer arrays hold).  0 / -1. */
int y2_train_prepare(network *net);
/* Floats of truth per image of a step: the inputs of a closing [cost]; l.truths = 150 behind a closing [region], 30 rows of
 * x, y, w, h, class in relative units, the list ended by the first x == 0; l.truths = side*side*(1+coords+classes) behind a
 * closing [detection], per cell is-object, the class row, x, y, w, h.  -1 (and y2_last_error) for a network the
 * trainer refuses; touches no device. */
int y2_train_truth_floats(network *net);
int y2_train_step(network *net, const float *x, const float *y, float *loss);            /* what train_network_datum calls */
int y2_train_step_device(network *net, const float *d_x, const float *d_y, float *loss); /* the inputs already in HBM */
/* The precision of the three products of every [convolutional] layer in a step (forward, input gradient, weight gradient).
 *   Y2_TRAIN_FP32    fp32 operands on the fp32 matrix cores: the default, and what a step always launched
 *   Y2_TRAIN_BF16X3  every operand value split into three bf16 numbers where it is staged, six bf16 products per fp32 product
 *                    (include/y2_split_rule.h): fp32 results but for terms below 2^-25 |a b|
 *   Y2_TRAIN_BF16    mixed precision: every operand value rounded once to bf16 (nearest even), fp32 accumulation
 * Nothing else of a step changes: batch norm, pooling, the heads, the cost, the update and the master weights stay fp32, no
 * buffer changes size, and everything the trainer refuses it still refuses (fp16 mode, y2_set_half, among it).  The mode is
 * the engine's, like the schedule: it may be set before y2_train_prepare or between steps and outlasts set_batch_network,
 * resize_network, y2_train_free and a new y2_train_prepare.  The environment variable Y2_TRAIN_PRECISION=fp32|bf16x3|bf16 sets
 * the default of networks parsed afterwards; another word fails parse_network_cfg.  y2_train_set_precision returns -1 (and
 * y2_last_error names the three modes) for any other value. */
enum { Y2_TRAIN_FP32 = 0, Y2_TRAIN_BF16X3 = 1, Y2_TRAIN_BF16 = 2 };
int y2_train_set_precision(network *net, int mode);
int y2_train_precision(network *net);
/* After a step the network is dirty: network_predict and every entry built on the forward pass, save_weights[_upto] and
 * y2_weights_arena first bring the masters (weights, biases, scales, rolling statistics) down into the host layer arrays
 * and re-pack the inference arena, so a caller that trains and then predicts or saves sees what it trained -- as with the
 * reference (y2_weights_arena uploads the arena before it hands it out, so a launcher that copies it itself gets the trained
 * weights).  y2_train_sync does that now.  A clean network does exactly what it did before.  set_batch_network,
 * resize_network and y2_denormalize_network sync and then drop the trainer (y2_train_free): train, set_batch_network(&net, 1),
 * predict keeps the steps, as with the reference.  load_weights and free_network drop it without a sync: the file's weights
 * replace the trained ones.  denormalize_convolutional_layer, which sees one layer and not the network, refuses while a
 * trainer exists. */
int y2_train_sync(network *net);
/* One array of layer `layer` as the reference holds it: activations as [batch][c][h][w], weights as [n][c][size][size]. */
enum { Y2_TRAIN_OUTPUT = 0, Y2_TRAIN_DELTA, Y2_TRAIN_X, Y2_TRAIN_X_NORM, Y2_TRAIN_MEAN, Y2_TRAIN_VARIANCE, Y2_TRAIN_MEAN_DELTA,
       Y2_TRAIN_VARIANCE_DELTA, Y2_TRAIN_WEIGHT_UPDATES, Y2_TRAIN_BIAS_UPDATES, Y2_TRAIN_SCALE_UPDATES, Y2_TRAIN_WEIGHTS,
       Y2_TRAIN_BIASES, Y2_TRAIN_SCALES, Y2_TRAIN_ROLLING_MEAN, Y2_TRAIN_ROLLING_VARIANCE,
       Y2_TRAIN_RAND /* [dropout]: the last step's draws, [batch][inputs]; its output and delta are the layer's in front */,
       Y2_TRAIN_STATE /* [rnn]: the state history, [time_steps + 1][B][hidden]; step t read slot t and wrote slot t + 1 */ };
/* An [rnn] layer's sub-layers, k = 0 input, 1 self, 2 output: Y2_TRAIN_SUB(k, what) names array `what` of sub-layer k.  Their
 * activations are [time_steps][B][outputs] (rows step-major); mean and variance are the last time step's, as in the reference
 * after a step.  The layer's own Y2_TRAIN_OUTPUT / Y2_TRAIN_DELTA are the output sub-layer's. */
#define Y2_TRAIN_SUB(k, what) ((((k) + 1) << 8) | (what))
int y2_train_pull(network *net, int layer, int what, float *dst, size_t n);
/* What forward_region_layer prints per call (region_layer.c:320), of the last step: the sums divided as in that printf, so
 * avg_iou, avg_class, avg_obj and recall are NaN when the batch held no truth.  The library prints nothing. */
typedef struct { float avg_iou, avg_class, avg_obj, avg_noobj, recall; int count, class_count; } y2_region_stats;
int y2_train_region_stats(network *net, int layer, y2_region_stats *out);
/* What forward_detection_layer prints per call (detection_layer.c:214), of the last step: Avg IOU, Pos Cat, All Cat, Pos Obj,
 * Any Obj and count, the sums divided as in that printf (all but avg_anyobj are NaN when no cell held an object). */
typedef struct { float avg_iou, avg_cat, avg_allcat, avg_obj, avg_anyobj; int count; } y2_detection_stats;
int y2_train_detection_stats(network *net, int layer, y2_detection_stats *out);
void y2_train_free(network *net);
/* The trainer's weight layout, [size][size][c][n], to and from the host's [n][c][size][size]: pure permutations. */
void y2_train_pack_weights(const float *ref, float *packed, int n, int c, int size);
void y2_train_unpack_weights(const float *packed, float *ref, int n, int c, int size);
/* The same for a dense ([connected]) layer's weights (y2h_train_dense_*): [outputs][inputs] on both sides, the K index
 * ci*h*w + y*w + x of the host (the layer in front is a c x h x w image) against (y*w + x)*c + ci of the dense NHWC activation
 * the device products read.  h = w = 1: the identity.  Pure permutations, no device. */
void y2_train_pack_dense_weights(const float *ref, float *packed, int outputs, int c, int h, int w);
void y2_train_unpack_dense_weights(const float *packed, float *ref, int outputs, int c, int h, int w);
/* ------------------------------------------------------------------------- */
/* The detection loader (data.c:664-714 load_data_detection): a training batch  */
/* is built from 8-bit frames and label rows.  The draws and the truth are made */
/* on the host, device-free (y2_aug.c); crop with jitter, the two-pass bilinear */
/* resize, flip, the HSV distortion and the clamp run as one kernel that writes */
/* the trainer's input where the step reads it.  The classifier loader          */
/* (load_data_augment: rotation) is built the same way, further down;           */
/* load_data_region stays with the caller.                                      */
/* ------------------------------------------------------------------------- */
/* One image of a batch: the frame as in y2_region (8-bit interleaved, h x w x c, `step` bytes between rows; channels
 * past the third are skipped), the draws of load_data_detection, and the label rows as the label file holds them,
 * boxes[nboxes][5] = id x y w h.  swaps[nboxes] are the indices randomize_boxes draws (row i is exchanged with row
 * swaps[i], i ascending); NULL means no shuffle.  The window (pleft, ptop, swidth x sheight) may reach outside the frame on
 * every side: edge pixels repeat (crop_image's constrain_int). */
typedef struct {
    const unsigned char *data; int h, w, c, step;
    int pleft, ptop, swidth, sheight, flip;
    float dhue, dsat, dexp;
    const float *boxes; int nboxes;
    const int *swaps;
} y2_aug_item;
/* The draws of one image, libc rand() called in exactly the reference's order: dw = (int)(ow * jitter), dh likewise; pleft,
 * pright, ptop, pbot = rand_uniform_strong(-dw, dw) .. truncated to int; flip = random_gen() % 2; dhue =
 * rand_uniform_strong(-hue, hue); dsat = rand_scale(saturation), dexp = rand_scale(exposure) (two calls each, 1. / scale in
 * double); then the nboxes indices of randomize_boxes, written to swaps[] when it is not NULL (drawn either way).  Fills
 * the draws of *item and sets item->swaps = swaps; the frame and the boxes of *item are not touched.  After srand(s),
 * y2_aug_random_paths for the batch and then this call image by image give the reference's single-threaded sequence.
 * (load_thread's `saturation == 0 -> 1`, `exposure == 0 -> 1` are the caller's: y2_net_augment reports what the cfg says.) */
void y2_aug_draw_detection(int ow, int oh, float jitter, float hue, float saturation, float exposure, int nboxes,
                           y2_aug_item *item, int *swaps);
void y2_aug_random_paths(int n, int m, int *out);    /* get_random_paths (data.c:42): out[i] = random_gen() % m */
int y2_aug_random_dim(void);                         /* detector.c:91-97, random=1: (rand() % 10 + 10) * 32; resize_network does the rest */
/* The truth row of one image, truth[5 * num_boxes] (num_boxes = 30 for a [region] head): zeroed; randomize_boxes with
 * item->swaps; correct_boxes with the dx, dy, 1./sx, 1./sy of data.c:693-707 in the reference's float / double promotions
 * (a row with x == 0 && y == 0 becomes 999999, the flip, the constrains); fill_truth_detection.  That function's quirk is
 * kept: a box whose corrected w or h is under .01 is skipped BUT KEEPS ITS SLOT, and the zero row it leaves ends the list for
 * the region layer, which stops at the first x == 0 -- the boxes behind it are not trained on, as in the reference.
 * 0, or -1 (y2_last_error) for a bad item.  Touches no device. */
int y2_aug_truth_detection(const y2_aug_item *item, int num_boxes, float *truth);
/* What train_detector reads of the cfg: jitter and random of the closing [region] layer, [net] hue / saturation / exposure
 * (parser.c:532-534, defaults 0 / 1 / 1).  Any pointer may be NULL.  -1 for a network that does not end in [region]. */
int y2_net_augment(network net, float *jitter, float *hue, float *saturation, float *exposure, int *random);
/* load_data_detection's pixel and truth work for one batch, n == net.batch items, into the trainer (prepared lazily, as by
 * train_network_datum): only the source rows and columns each window touches, the descriptor table and the n * 150 truth
 * floats are packed into one pinned staging buffer and go up in one copy; one kernel writes the trainer's NHWC input, the
 * truth is copied beside it.  The call returns once the copy has left the staging buffer.  Channel k of the input is byte
 * k of a pixel, 2 - k with swap_rb (BGR frames).  Refused before any allocation, upload or launch, the item named in
 * y2_last_error(): n != net.batch, net.c != 3, a network that does not end in [region] or that the trainer refuses, NULL
 * data, c < 3, step < w * c, a frame without pixels, swidth < 1 or sheight < 1, nboxes < 0, nboxes > 0 with NULL boxes, a
 * swap index outside the rows. */
int y2_train_load_detection(network *net, const y2_aug_item *items, int n, int swap_rb);
/* ---- the classifier loader (data.c:870-879 load_data_augment): rotated, scaled, aspect-stretched bilinear crop,
 * flip, HSV distortion, the label row.  PINNED to the compiled reference, run whole through recording stubs
 * (tests/golden/aug_cls.npz): the rand primitives, the sequence around them (paths, the per-image call order, the flip
 * draw between the two image calls), the label and hierarchy rows.  RESTATED only (image.c does not compile without
 * OpenCV): the order of the five draws in random_augment_image and the three in random_distort_image, the arithmetic
 * between them, and the pixel chain, which is held to tests/aug_cls_rule.py by array_equal. ---- */
/* One image: the frame as in y2_aug_item, what random_augment_image hands to rotate_crop_image (image.c:1702), the flip
 * and the distortion. */
typedef struct {
    const unsigned char *data; int h, w, c, step;
    float aspect, scale, rad, dx, dy;
    int flip;
    float dhue, dsat, dexp;
} y2_aug_cls_item;
/* The draws of one image of load_image_augment_paths for an ow x oh frame, libc rand() called in the reference's order:
 * aspect = rand_scale(aspect); r = rand_int(min, max); int m = (oh < ow*aspect) ? oh : ow*aspect (truncated);
 * scale = (float)r / m; rad = rand_uniform(-angle, angle) * TWO_PI / 360. (in double, rounded once);
 * dx = (ow*scale/aspect - size) / 2., dy = (oh*scale - size) / 2., each clamped at 0, then rand_uniform(-dx, dx),
 * rand_uniform(-dy, dy); flip = random_gen() % 2; dhue = rand_uniform_strong(-hue, hue); dsat = rand_scale(saturation);
 * dexp = rand_scale(exposure) -- a bound below 1 goes through rand_uniform_strong's swap.  Fills the draws of *item; the
 * frame fields are not touched.  -1 when the truncated m is 0 (the reference divides by it); every draw is still made, so
 * the sequence stays the reference's.  After srand(s), y2_aug_random_paths for the batch and then this call image by image
 * give the reference's single-threaded sequence. */
int y2_aug_draw_classification(int ow, int oh, int min, int max, int size, float angle, float aspect, float hue,
                               float saturation, float exposure, y2_aug_cls_item *item);
/* fill_truth (data.c:387): truth[i] = 1 where labels[i] occurs in path (strstr), 0 elsewhere; with a hierarchy,
 * fill_hierarchy (data.c:401): every ancestor of a set entry is set, and each group without a set member is filled with
 * the reference's SECRET_NUM (-1234).  Returns the number of labels that matched (the reference prints when it is not 1;
 * nothing is printed here), -1 for NULL arguments.  On the host, like hierarchy_predictions: the trainer refuses a tree
 * softmax. */
int y2_aug_labels(const char *path, char **labels, int k, const tree *hierarchy, float *truth);
/* What train_classifier reads of the [net] section (parser.c:527-534): min_crop (default net.w), max_crop (net.w * 2),
 * angle (0), aspect (1), hue (0), saturation (1), exposure (1).  Any pointer may be NULL.  -1 without an engine. */
int y2_net_augment_classifier(network net, int *min_crop, int *max_crop, float *angle, float *aspect, float *hue,
                              float *saturation, float *exposure);
/* load_data_augment's pixel work for one batch, n == net.batch items, into the trainer, staged as
 * y2_train_load_detection stages: the frame rectangle each image's taps can touch, the descriptor table and `truth`
 * ([n][inputs of the closing [cost] layer], as y2_train_step takes it) go up in one copy from one pinned buffer, one
 * kernel writes the net.w x net.w NHWC input (size = net.w, as args.size in train_classifier), the truth is copied beside
 * it.  Refused before any allocation, upload or launch, by name in y2_last_error(): n != net.batch, net.c != 3,
 * net.h != net.w (the reference would hand the network a batch of the wrong length), a network that ends in [region] or
 * that the trainer refuses, NULL truth or data, c < 3, step < w * c, a frame without pixels, a scale or aspect that is
 * not finite and positive, a rad, dx or dy that is not finite.  A refused load leaves nothing loaded. */
int y2_train_load_classification(network *net, const y2_aug_cls_item *items, const float *truth, int n, int swap_rb);
/* get_rnn_data (rnn.c:86-114): x and y are [steps*batch][characters], zeroed here; row j*batch + i holds the one-hot of the
 * byte stream i reads at its step j (x) and of the byte behind it (y); offsets[i] advances by one per step, modulo len.
 * Where the reference calls error("Bad char") half-way -- a zero byte -- this returns -1 with that message (y2_last_error)
 * BEFORE anything is written or any offset moves; a byte >= characters, which the reference would write out of bounds, is
 * refused the same way. */
int y2_get_rnn_data(const unsigned char *text, size_t *offsets, int characters, size_t len, int batch, int steps, float *x, float *y);
/* The same on the device, into the trainer's input and truth: the B x (time_steps + 1) bytes the B = net.batch / time_steps
 * streams read go up (not 2 x net.batch x inputs floats), one kernel writes both one-hot tensors, offsets advance as
 * get_rnn_data's.  For a network whose first layer is an [rnn] and whose [cost] has as many values as the network reads.
 * Refused by name, nothing loaded and no offset moved: a network the trainer refuses, a zero byte or one >= inputs. */
int y2_train_load_rnn_data(network *net, const unsigned char *text, size_t len, size_t *offsets);
/* step_on_device on what y2_train_load_detection or y2_train_load_classification loaded; a second step on the same load is
 * allowed.  Refused with nothing loaded, and after set_batch_network / resize_network dropped the trainer (load again). */
int y2_train_step_loaded(network *net, float *loss);
/* The loaded input as [batch][3][h][w] and the truth ([batch][150] behind a [region] head, [batch][y2_train_truth_floats]
 * for a classifier), either may be NULL: for tests and callers that look. */
int y2_train_pull_input(network *net, float *x_nchw, float *truth);
/* Host wall time of the last y2_train_load_detection / y2_train_load_classification in ms: ms[0] pack (pixels, table,
 * truth), ms[1] enqueueing the copy, the kernel and the truth copy, ms[2] waiting for the copy to leave the staging buffer. */
int y2_train_load_times(network *net, float *ms);

/* ------------------------------------------------------------------------ */
/* Dreaming: nightmare.c's optimize_picture / run_nightmare (y2_dream.c).      */
/* The gradient of a layer's activations with respect to the input picture,  */
/* climbed on a picture that stays in HBM.  A context is opened on a loaded  */
/* batch-1 network and a picture ([c][h][w] floats, c as the network's); the */
/* picture is uploaded once, every step reads and writes it there, the host  */
/* sees it on y2_dream_fetch.  The context packs the weights of the layers   */
/* it needs once (again after load_weights, y2_denormalize_network or        */
/* training steps changed them) and keeps per input size the activations,    */
/* deltas and maxpool winners of the truncated network, at most eight sizes, */
/* least recently used dropped.  It NEVER resizes or truncates the caller's  */
/* network (the reference leaves net->n, w, h changed; here network_predict  */
/* gives the bytes it gave before).  Accepted: [convolutional] without       */
/* batch_normalize, stride 1, linear / leaky / logistic / relu, and          */
/* [maxpool]; everything else is refused by name before any allocation.      */
/* Weight and bias gradients are not computed: the reference accumulates     */
/* them and never applies them.  -reconstruct is out of scope.               */
/* ------------------------------------------------------------------------ */
typedef struct y2_dream y2_dream;
typedef struct { int layer_offset, octave, dx, dy, flip; } y2_dream_draws;
/* selected: values of the last layer the last step kept (0: the gradient was all zero, and with norm the picture is NaN now,
 * as in the reference); bytes copied since open; device allocations since open; steps since open */
typedef struct { int selected; unsigned long long h2d_bytes, d2h_bytes; unsigned long allocations, steps; } y2_dream_counters;
/* the five rand() calls of one run_nightmare iteration in its order: rand()%range - range/2 (add max_layer), rand()%octaves,
 * rand()%16 - 8, rand()%16 - 8, rand()%2 */
void y2_dream_draw(int range, int octaves, y2_dream_draws *out);
float y2_dream_scale(int octave);                                        /* 1/pow(1.33333333, octave), as a float argument */
void y2_dream_size(int w, int h, float scale, int *ow, int *oh);         /* (int)(w*scale), (int)(h*scale) */
/* Every refusal of a step at (max_layer, scale) on a c x h x w picture, by name ("dream: layer %d (%s): ..."), without a
 * device call: what y2_dream_step, optimize_picture and y2_nightmare ask before they allocate.  0, or -1 after y2_fail. */
int y2_dream_check(network *net, int max_layer, int c, int h, int w, float scale);
y2_dream *y2_dream_open(network *net, const float *picture, int c, int h, int w);
int y2_dream_step(y2_dream *d, int max_layer, float scale, float rate, float thresh, int norm, int dx, int dy, int flip);
/* run_nightmare's round end: rotate_image when rotate != 0, crop_image by zoom with its float-to-int truncations, resize back */
int y2_dream_round_end(y2_dream *d, float rotate, float zoom);
int y2_dream_fetch(y2_dream *d, float *picture);
int y2_dream_stats(y2_dream *d, y2_dream_counters *out);
/* For tests and callers that look, of the last step: Y2_DREAM_OUTPUT / Y2_DREAM_DELTA of layer `layer` as [c][h][w];
 * Y2_DREAM_INPUT (the network input the step built) and Y2_DREAM_GRADIENT (the image gradient) as [c][h][w] at the step's
 * size; Y2_DREAM_UPDATE, the picture-sized update before normalisation.  n must be the array's size. */
enum { Y2_DREAM_OUTPUT = 0, Y2_DREAM_DELTA, Y2_DREAM_INPUT, Y2_DREAM_GRADIENT, Y2_DREAM_UPDATE };
int y2_dream_pull(y2_dream *d, int layer, int what, float *dst, size_t n);
void y2_dream_close(y2_dream *d);
/* The reference's entry point with its own three rand() draws: uploads orig, steps, fetches into orig.data.  The context is
 * cached on the network (reopened when the picture's size changes) and freed by free_network. */
void optimize_picture(network *net, image orig, int max_layer, float scale, float rate, float thresh, int norm);
/* Seeding: the draws are libc's rand().  The HIP runtime draws from the same generator while it starts up at the first device
 * work of a process, so call srand() after that (after a y2_dream_open, a network_predict, ...), not before it, when the
 * sequence matters. */
/* run_nightmare's loop without file I/O and without srand: rounds x iters steps with its draws, one fetch per round into
 * im.data, then per_round(round, im, user) if given, then the round end.  Returns 0, or -1 after y2_fail. */
int y2_nightmare(network *net, image im, int max_layer, int range, int norm, int rounds, int iters, int octaves, float zoom,
                 float rate, float thresh, float rotate, void (*per_round)(int round, image im, void *user), void *user);

/* ------------------------------------------------------------------------ */
/* Go: go.c's entry points and the batched calls under them (y2_go.c).        */
/* ------------------------------------------------------------------------ */
/* A board is 361 floats holding exactly 0, 1 or -1, row-major (board[row*19+col]); a packed board or ko string is 91 bytes
 * (four points per byte, bit 2j = 1, bit 2j+1 = -1); a record is 93 bytes: row, column, the packed board seen by the mover.
 * Device-free, under the reference's names and signatures: */
typedef struct { char **data; int n; } moves;                    /* go.c:16-19 */
void string_to_board(char *s, float *board);                     /* go.c:56 */
void board_to_string(char *s, float *board);                     /* go.c:75 */
void flip_board(float *board);                                   /* go.c:254 */
int *calculate_liberties(float *board);                          /* go.c:188: calloc'ed, the caller frees */
void move_go(float *b, int p, int r, int c);                     /* go.c:304 */
int suicide_go(float *b, int p, int r, int c);                   /* go.c:326 */
int legal_go(float *b, char *ko, int p, int r, int c);           /* go.c:338: does NOT reject suicide */
void print_board(float *board, int swap, int *indexes);          /* go.c:208: to stderr; indexes NULL or five points */
/* go.c:34: a file of 94-byte lines (the 93-byte record and the newline self_go prints behind it); data[i] holds line i.  The
 * count is not printed.  A file that cannot be opened is an error (y2_last_error), n = 0. */
moves load_go_moves(char *filename);
void y2_go_free_moves(moves m);
/* random_go_moves' draws (go.c:97-105) for one batch, in its order: rand() % n_records, rand() % 2, rand() % 4 per item. */
int y2_go_draw_moves(int n_records, int batch, int *pick, int *flip, int *rot);
/* The reference's two device entries.  predict_move (go.c:262): the network on the board and, with multi, on its seven
 * other dihedral views, summed in the reference's order and scaled by 1/8, occupied points zeroed.  generate_move (go.c:351)
 * writes temp on every layer, draws its one uniform with libc rand() exactly as rand_uniform(0, 1) does -- on every call
 * that is not refused, also when it returns -1 -- and returns the point, or -1 when the best point is suicide.  The board
 * comes back unchanged.  A refused call also returns -1 (y2_last_error). */
void predict_move(network net, float *board, float *move, int multi);
int generate_move(network net, int player, float *board, int multi, float thresh, float temp, char *ko, int print);
/* The batched entries.  All of them refuse, by the argument's name in y2_last_error() and before any device work: a network
 * that does not read 19 x 19 x 1 or does not give 361 values, fp16 mode, n <= 0, a board value other than 0 / 1 / -1, a
 * player other than 1 / -1.  Any n is taken: rows beyond net.batch are forwarded net.batch rows at a time (the network is
 * never re-planned; set_batch_network(&net, 8 * n) first makes a multi move one forward).
 *   y2_go_predict   moves[n][361] = predict_move of each board as seen by players[i] (a -1 negates it first)
 *   y2_go_rules     liberties[n][361] ints, legal[n][361] and suicide[n][361] bytes (any may be NULL) of the positions
 *                   (boards as they are, ko[n][91], players); the network only supplies the device and stream
 *   y2_go_generate  generate_move for n positions in one chain -- views, forward, merge, rules, pick -- and one sync:
 *                   index[n]; kept (or NULL) receives the thresholded arrays [n][361] the samples were drawn from.
 *                   Position i uses uniforms[i]; temp is written on every layer.
 *   y2_go_valid     valid_go's loop (go.c:421-431): predicted[i] = max_index(predict_move(board of record i)); records is
 *                   [n][93].  The caller compares with records[i][0] * 19 + records[i][1].
 *   y2_go_selfplay  self_go's loop (go.c:775-823) for `games` games in lockstep from empty boards and zeroed ko strings (the
 *                   reference keeps its two strings from one game into the next; here every call starts clean).  Per ply:
 *                   one forward over all games, the rules, the pick, the move.  first = 0: net moves first, 1: net2 does;
 *                   all games share it, so a ply uses one network (net2 may be the same network).  Game g's ply t uses
 *                   uniforms[g*max_moves+t].  records[games][max_moves][93] holds, per move made, the reference's record
 *                   (row, column, the board packed from the mover's side, before the move); counts[g] how many.  A game
 *                   ends at -1 or at max_moves (the reference's cap is 300); an ended game's records and board no longer
 *                   change.  final_boards[games][361] or NULL.  With two different networks every ply ends in a host
 *                   wait; with one network the call waits once at its end and once every 16 plies, where it asks whether a
 *                   game is still alive and returns when none is (y2_go_set_poll(net, every) changes the interval, 0:
 *                   never asked).  The results do not depend on it. */
int y2_go_predict(network net, const float *boards, const int *players, int n, int multi, float *moves);
int y2_go_rules(network net, const float *boards, const char *ko, const int *players, int n, int *liberties, unsigned char *legal,
                unsigned char *suicide);
int y2_go_generate(network net, const float *boards, const char *ko, const int *players, int n, int multi, float thresh, float temp,
                   const float *uniforms, int *index, float *kept);
int y2_go_valid(network net, const unsigned char *records, int n, int multi, int *predicted);
int y2_go_selfplay(network net, network net2, int games, int first, int max_moves, int multi, float thresh, float temp,
                   const float *uniforms, unsigned char *records, int *counts, float *final_boards);
int y2_go_set_poll(network net, int every);
/* train_go's input (random_go_moves, go.c:92-115) built in the trainer on the device, staged like the other loaders: the
 * net.batch picked records and the draws go up in one copy, one kernel writes input and truth.  Per item: decode record
 * pick[i], the one-hot label at (row, col), the board cleared at that point, flip_image on both when flip[i], then
 * rotate_image_cw(rot[i]) on both -- flip first, the opposite of predict_move's views.  records is [n_records][93].
 * Refused by name with nothing loaded: a network that is not 19 x 19 x 1 with a 361-value [cost], one the trainer refuses,
 * a pick outside the records, a flip other than 0 / 1, a rot outside 0..3, a picked record whose row or column is outside
 * 0..18.  y2_train_step_loaded steps on it. */
int y2_train_load_go(network *net, const unsigned char *records, int n_records, const int *pick, const int *flip, const int *rot);

/* Copy layer i's activations to host as NCHW [batch][out_c][out_h][out_w] (or [batch][outputs]). */
int y2_pull_layer_output(network net, int i, float *dst);
/* Per-layer device time of the last forward in ms (needs y2_set_timing(net,1)); returns layers written. */
void y2_set_timing(network *net, int on);
int y2_layer_times_ms(network net, float *ms, int max_layers);
/* Name of the kernel a layer runs ("conv_mfma_f32_128x128x32_k3", "maxpool", ...). */
const char *y2_layer_kernel(network net, int i);
/* Stream the engine launches on (hipStream_t) and a whole-device sync. */
void *y2_stream(network net);
void y2_sync(network net);
/* Last error text of the library (never NULL). */
const char *y2_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* SR_YOLO2_H */
