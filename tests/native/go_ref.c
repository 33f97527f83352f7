/* Driver for the Go fixtures (tests/golden/gen_go_golden.py): linked with the reference's go.c, compiled where it lies,
 * and with the reference library.  It calls go.c's functions as they stand and records what they return.
 *
 * go.c needs three functions of the reference's image.c, which has no compiled form without OpenCV; they are stated here
 * (float_to_image, flip_image, rotate_image_cw) and the generator asserts them against numpy.rot90 / fliplr.
 *
 * Four functions are wrapped so that values inside generate_move can be seen without changing it -- each wrapper calls
 * the real one (RTLD_NEXT) and only records: rand (the raw draws), rand_uniform (the uniform sample_array drew),
 * sum_array (its argument is the thresholded array, before sample_array scales it), network_predict (returns a preset
 * row when one is set: the pick cases; otherwise the real forward).
 *
 *   go_ref image OUT                       the three image functions on an asymmetric 19x19 array
 *   go_ref rules IN OUT                    calculate_liberties, legal_go x 361, suicide_go x 361 per position
 *   go_ref moves IN OUT                    move_go + board_to_string per (board, player, row, col)
 *   go_ref load FILE OUT                   load_go_moves
 *   go_ref batch FILE SEED N OUT           random_go_moves(m, boards, labels, N) after srand(SEED), and its raw draws
 *   go_ref pick IN OUT                     generate_move on preset rows
 *   go_ref net CFG WEIGHTS IN OUT          predict_move / generate_move / a game / valid_go's loop on a real network
 *   go_ref time IN                         ms per (361 legal_go + 2 suicide_go) on each position of IN
 */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "network.h"
#include "parser.h"
#include "utils.h"

typedef struct { char **data; int n; } moves;
moves load_go_moves(char *filename);
void string_to_board(char *s, float *board);
void board_to_string(char *s, float *board);
void random_go_moves(moves m, float *boards, float *labels, int n);
int *calculate_liberties(float *board);
void flip_board(float *board);
void predict_move(network net, float *board, float *move, int multi);
void move_go(float *b, int p, int r, int c);
int suicide_go(float *b, int p, int r, int c);
int legal_go(float *b, char *ko, int p, int r, int c);
int generate_move(network net, int player, float *board, int multi, float thresh, float temp, char *ko, int print);

/* ---- the three image.c functions go.c calls ---- */
image float_to_image(int w, int h, int c, float *data)
{
    image out;
    out.w = w; out.h = h; out.c = c; out.data = data;
    return out;
}

void flip_image(image a)                                 /* columns mirrored */
{
    int k, i, j;
    for (k = 0; k < a.c; ++k)
        for (i = 0; i < a.h; ++i)
            for (j = 0; j < a.w / 2; ++j) {
                float *row = a.data + (size_t)a.w * (i + a.h * k), t = row[j];
                row[j] = row[a.w - 1 - j]; row[a.w - 1 - j] = t;
            }
}

void rotate_image_cw(image im, int times)               /* one turn: new[r][c] = old[c][n-1-r] */
{
    const int n = im.w;
    float *tmp = malloc((size_t)n * n * sizeof(float));
    int t, k, r, c;
    times = (times + 400) % 4;
    for (t = 0; t < times; ++t)
        for (k = 0; k < im.c; ++k) {
            float *a = im.data + (size_t)n * n * k;
            memcpy(tmp, a, (size_t)n * n * sizeof(float));
            for (r = 0; r < n; ++r) for (c = 0; c < n; ++c) a[r * n + c] = tmp[c * n + (n - 1 - r)];
        }
    free(tmp);
}

/* ---- recording wrappers ---- */
static int g_raw[4096], g_nraw;
static float g_uniform, g_kept[361], *g_preset;
static int g_have_kept;

int rand(void)
{
    static int (*real)(void);
    int v;
    if (!real) real = (int (*)(void))dlsym(RTLD_NEXT, "rand");
    v = real();
    if (g_nraw < 4096) g_raw[g_nraw++] = v;
    return v;
}

float rand_uniform(float min, float max)
{
    static float (*real)(float, float);
    if (!real) real = (float (*)(float, float))dlsym(RTLD_NEXT, "rand_uniform");
    return g_uniform = real(min, max);
}

float sum_array(float *a, int n)
{
    static float (*real)(float *, int);
    if (!real) real = (float (*)(float *, int))dlsym(RTLD_NEXT, "sum_array");
    if (n == 361) { memcpy(g_kept, a, sizeof g_kept); g_have_kept = 1; }
    return real(a, n);
}

float *network_predict(network net, float *input)
{
    static float *(*real)(network, float *);
    if (g_preset) return g_preset;
    if (!real) real = (float *(*)(network, float *))dlsym(RTLD_NEXT, "network_predict");
    return real(net, input);
}

/* ---- plumbing ---- */
static FILE *open_or_die(const char *path, const char *mode)
{
    FILE *f = fopen(path, mode);
    if (!f) { fprintf(stderr, "go_ref: cannot open %s\n", path); exit(2); }
    return f;
}
static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "go_ref: short read\n"); exit(2); } }
static void wr(FILE *f, const void *p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { fprintf(stderr, "go_ref: short write\n"); exit(2); } }
static int rd_int(FILE *f) { int v; rd(f, &v, sizeof v); return v; }
static float rd_float(FILE *f) { float v; rd(f, &v, sizeof v); return v; }
static void wr_int(FILE *f, int v) { wr(f, &v, sizeof v); }

static void rules_of(float *board, char *ko, int player, int *lib, unsigned char *legal, unsigned char *suicide)
{
    int *l = calculate_liberties(board), r, c;
    memcpy(lib, l, 361 * sizeof(int));
    free(l);
    for (r = 0; r < 19; ++r) for (c = 0; c < 19; ++c) {
        legal[r * 19 + c] = (unsigned char)legal_go(board, ko, player, r, c);
        suicide[r * 19 + c] = (unsigned char)suicide_go(board, player, r, c);
    }
}

static int cmd_image(const char *out)
{
    FILE *f = open_or_die(out, "wb");
    float a[361], b[361];
    int i, t;
    for (i = 0; i < 361; ++i) a[i] = (float)i;
    for (t = -7; t <= 7; ++t) {
        memcpy(b, a, sizeof b);
        rotate_image_cw(float_to_image(19, 19, 1, b), t);
        wr(f, b, sizeof b);
    }
    memcpy(b, a, sizeof b);
    flip_image(float_to_image(19, 19, 1, b));
    wr(f, b, sizeof b);
    fclose(f);
    return 0;
}

static int cmd_rules(const char *in, const char *out)
{
    FILE *f = open_or_die(in, "rb"), *o = open_or_die(out, "wb");
    int n = rd_int(f), i;
    for (i = 0; i < n; ++i) {
        float board[361], before[361];
        char ko[91];
        int player, lib[361];
        unsigned char legal[361], suicide[361];
        rd(f, board, sizeof board); rd(f, ko, 91); player = rd_int(f);
        memcpy(before, board, sizeof board);
        rules_of(board, ko, player, lib, legal, suicide);
        if (memcmp(before, board, sizeof board)) { fprintf(stderr, "go_ref: position %d changed under legal_go\n", i); return 3; }
        wr(o, lib, sizeof lib); wr(o, legal, 361); wr(o, suicide, 361);
    }
    fclose(f); fclose(o);
    return 0;
}

static int cmd_moves(const char *in, const char *out)
{
    FILE *f = open_or_die(in, "rb"), *o = open_or_die(out, "wb");
    int n = rd_int(f), i;
    for (i = 0; i < n; ++i) {
        float board[361];
        char s[91];
        int player, r, c;
        rd(f, board, sizeof board); player = rd_int(f); r = rd_int(f); c = rd_int(f);
        move_go(board, player, r, c);
        board_to_string(s, board);
        wr(o, board, sizeof board); wr(o, s, 91);
    }
    fclose(f); fclose(o);
    return 0;
}

static int cmd_load(char *file, const char *out)
{
    FILE *o = open_or_die(out, "wb");
    moves m = load_go_moves(file);
    int i;
    wr_int(o, m.n);
    for (i = 0; i < m.n; ++i) wr(o, m.data[i], 93);
    fclose(o);
    return 0;
}

static int cmd_batch(char *file, int seed, int n, const char *out)
{
    FILE *o = open_or_die(out, "wb");
    moves m = load_go_moves(file);
    float *boards = calloc((size_t)361 * n, sizeof(float)), *labels = calloc((size_t)361 * n, sizeof(float));
    srand(seed);
    g_nraw = 0;
    random_go_moves(m, boards, labels, n);
    wr_int(o, g_nraw); wr(o, g_raw, (size_t)g_nraw * sizeof(int));
    wr(o, boards, (size_t)361 * n * sizeof(float)); wr(o, labels, (size_t)361 * n * sizeof(float));
    fclose(o);
    return 0;
}

/* one generate_move with everything it leaves behind: index, the uniform, the thresholded array, the board afterwards */
static void generate_and_record(FILE *o, network net, FILE *f)
{
    float board[361], before[361], thresh, temp;
    char ko[91];
    int seed, player, multi, index;
    seed = rd_int(f); player = rd_int(f); rd(f, board, sizeof board); multi = rd_int(f);
    thresh = rd_float(f); temp = rd_float(f); rd(f, ko, 91);
    memcpy(before, board, sizeof board);
    srand(seed);
    g_have_kept = 0; g_uniform = -1;
    index = generate_move(net, player, board, multi, thresh, temp, ko, 0);
    if (memcmp(before, board, sizeof board)) { fprintf(stderr, "go_ref: generate_move changed the board\n"); exit(3); }
    wr_int(o, index); wr(o, &g_uniform, sizeof g_uniform); wr(o, g_kept, sizeof g_kept);
}

static int cmd_pick(const char *in, const char *out)
{
    FILE *f = open_or_die(in, "rb"), *o = open_or_die(out, "wb");
    network net;
    int n = rd_int(f), i;
    float row[361];
    memset(&net, 0, sizeof net);                         /* n = 0 layers: the temperature loop writes nothing */
    for (i = 0; i < n; ++i) {
        rd(f, row, sizeof row);
        g_preset = row;
        generate_and_record(o, net, f);
        g_preset = NULL;
    }
    fclose(f); fclose(o);
    return 0;
}

static int cmd_net(char *cfg, char *weights, const char *in, const char *out)
{
    FILE *f = open_or_die(in, "rb"), *o = open_or_die(out, "wb");
    network net = parse_network_cfg(cfg);
    int op;
    load_weights(&net, weights);
    set_batch_network(&net, 1);
    while (fread(&op, sizeof op, 1, f) == 1) {
        if (op == 1) {                                   /* predict_move(board, multi) */
            float board[361], move[361];
            int multi;
            rd(f, board, sizeof board); multi = rd_int(f);
            predict_move(net, board, move, multi);
            wr(o, move, sizeof move);
        } else if (op == 2) {
            int i;
            generate_and_record(o, net, f);
            for (i = 0; i < net.n; ++i) wr(o, &net.layers[i].temperature, sizeof(float));
        } else if (op == 3) {                            /* one game, driven as go.c:775-823 drives it */
            float *board = calloc(361, sizeof(float)), thresh, temp;
            char *one = calloc(91, 1), *two = calloc(91, 1), rec[93];
            int seed = rd_int(f), plies = rd_int(f), multi = rd_int(f), player = 1, count = 0;
            thresh = rd_float(f); temp = rd_float(f);
            srand(seed);
            wr_int(o, plies);
            while (count < plies) {
                int index = generate_move(net, player, board, multi, thresh, temp, two, 0), row, col;
                char *swap;
                wr_int(o, index); wr(o, &g_uniform, sizeof g_uniform);
                if (index < 0) break;
                row = index / 19; col = index % 19;
                swap = two; two = one; one = swap;
                if (player < 0) flip_board(board);
                rec[0] = row; rec[1] = col;
                board_to_string(rec + 2, board);
                if (player < 0) flip_board(board);
                ++count;
                wr(o, rec, 93);
                move_go(board, player, row, col);
                board_to_string(one, board);
                player = -player;
            }
            wr_int(o, -2);                               /* end of game */
            wr_int(o, count); wr(o, board, 361 * sizeof(float));
            free(board); free(one); free(two);
        } else if (op == 4) {                            /* valid_go's loop body (go.c:421-428) */
            float board[361], move[361];
            char rec[93];
            int multi;
            rd(f, rec, 93); multi = rd_int(f);
            string_to_board(rec + 2, board);
            predict_move(net, board, move, multi);
            wr_int(o, max_index(move, 361));
        } else { fprintf(stderr, "go_ref: op %d\n", op); return 2; }
    }
    fclose(f); fclose(o);
    return 0;
}

static int cmd_time(const char *in)
{
    FILE *f = open_or_die(in, "rb");
    int n = rd_int(f), i;
    for (i = 0; i < n; ++i) {
        float board[361];
        char ko[91];
        int player, rep, r, c, reps = 0, sink = 0;
        struct timespec t0, t1;
        double ms = 0;
        rd(f, board, sizeof board); rd(f, ko, 91); player = rd_int(f);
        for (rep = 0; rep < 3; ++rep)                    /* warm-up */
            for (r = 0; r < 19; ++r) for (c = 0; c < 19; ++c) sink += legal_go(board, ko, player, r, c);
        while (ms < 300 || reps < 20) {                  /* what generate_move runs per call: 361 legal_go, 2 suicide_go */
            clock_gettime(CLOCK_MONOTONIC, &t0);
            for (r = 0; r < 19; ++r) for (c = 0; c < 19; ++c) sink += legal_go(board, ko, player, r, c);
            sink += suicide_go(board, player, 3, 3) + suicide_go(board, player, 15, 15);
            clock_gettime(CLOCK_MONOTONIC, &t1);
            ms += (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) * 1e-6;
            ++reps;
        }
        printf("position %d: %.4f ms per move (%d repeats, sink %d)\n", i, ms / reps, reps, sink);
    }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "image")) return cmd_image(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "rules")) return cmd_rules(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "moves")) return cmd_moves(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "load")) return cmd_load(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "batch")) return cmd_batch(argv[2], atoi(argv[3]), atoi(argv[4]), argv[5]);
    if (argc == 4 && !strcmp(argv[1], "pick")) return cmd_pick(argv[2], argv[3]);
    if (argc == 6 && !strcmp(argv[1], "net")) return cmd_net(argv[2], argv[3], argv[4], argv[5]);
    if (argc == 3 && !strcmp(argv[1], "time")) return cmd_time(argv[2]);
    fprintf(stderr, "usage: go_ref image|rules|moves|load|batch|pick|net|time ...\n");
    return 2;
}
