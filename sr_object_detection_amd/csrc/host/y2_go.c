/*
 * Go: the reference's go.c entry points (string_to_board :56, board_to_string :75, calculate_liberties :188, print_board
 * :208, flip_board :254, predict_move :262, move_go :304, suicide_go :326, legal_go :338, generate_move :351,
 * load_go_moves :34) and the batched y2_go_* calls the two device entries are written on.
 *
 * The reference runs eight batch-1 forwards per predicted move, turning the board and each output row on the host, and
 * then 361 legal_go calls -- each a calculate_liberties that flood-fills from every empty point -- plus top_k, the
 * threshold, max_index, sample_array and up to two suicide_go calls.  Here a move is one chain of launches on the
 * engine's stream: the views kernel writes the network input, the forward runs at whatever batch the network has,
 * the merge kernel un-turns and sums the rows, the rules kernel gives the legal and suicide maps of every position, the
 * pick kernel decides.  One sync at the end brings n ints down.  Self-play keeps boards, ko strings and records in
 * HBM and runs G games in lockstep.
 *
 * Rows beyond the network's batch are processed in chunks of net.batch rows (the network is never re-planned here:
 * callers that want one forward per move set the batch to 8 * n with set_batch_network first).
 *
 * The first half of the file is device-free.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

enum { GO_P = 361, GO_KO = 91, GO_REC = 93, GO_LINE = 94 };

/* ------------------------------------------------------------------ */
/* the rules on the host (device-free)                                 */
/* ------------------------------------------------------------------ */
void string_to_board(char *s, float *board)
{
    int p;
    for (p = 0; p < GO_P; ++p) {
        const int two = ((unsigned char)s[p >> 2] >> (2 * (p & 3))) & 3;
        board[p] = (two & 1) ? 1 : (two & 2) ? -1 : 0;          /* `me` is tested first */
    }
}

void board_to_string(char *s, float *board)
{
    int p;
    memset(s, 0, GO_KO);
    for (p = 0; p < GO_P; ++p) {
        if (board[p] == 1) s[p >> 2] |= 1 << (2 * (p & 3));
        if (board[p] == -1) s[p >> 2] |= 2 << (2 * (p & 3));
    }
}

void flip_board(float *board)
{
    int i;
    for (i = 0; i < GO_P; ++i) board[i] = -board[i];
}

/* the group of the stone at `start` by an explicit stack; member[] marks it, returns its size */
static int go_group(const float *board, int start, unsigned char *member, int *stack)
{
    const float side = board[start];
    int top = 0, size = 0;
    memset(member, 0, GO_P);
    member[start] = 1; stack[top++] = start;
    while (top) {
        const int p = stack[--top], r = p / 19, c = p % 19;
        int q[4], k;
        ++size;
        q[0] = r < 18 ? p + 19 : -1; q[1] = r > 0 ? p - 19 : -1; q[2] = c < 18 ? p + 1 : -1; q[3] = c > 0 ? p - 1 : -1;
        for (k = 0; k < 4; ++k)
            if (q[k] >= 0 && !member[q[k]] && board[q[k]] == side) { member[q[k]] = 1; stack[top++] = q[k]; }
    }
    return size;
}

int *calculate_liberties(float *board)
{
    int *lib = calloc(GO_P, sizeof(int)), stack[GO_P], p, k;
    unsigned char member[GO_P], done[GO_P];
    if (!lib) return NULL;
    memset(done, 0, sizeof done);
    for (p = 0; p < GO_P; ++p) {
        int count = 0, e;
        if (board[p] == 0 || done[p]) continue;
        go_group(board, p, member, stack);
        /* an empty point counts once for the group however many of its stones it touches (the per-point `visited`) */
        for (e = 0; e < GO_P; ++e) {
            const int r = e / 19, c = e % 19;
            if (board[e] != 0) continue;
            if ((c > 0 && member[e - 1]) || (c < 18 && member[e + 1]) || (r > 0 && member[e - 19]) || (r < 18 && member[e + 19])) ++count;
        }
        for (k = 0; k < GO_P; ++k) if (member[k]) { lib[k] = count; done[k] = 1; }
    }
    return lib;
}

static void remove_group(float *b, const int *lib, int p, int at)
{
    unsigned char member[GO_P];
    int stack[GO_P], k;
    if (at < 0 || b[at] != p || lib[at] != 1) return;
    go_group(b, at, member, stack);
    for (k = 0; k < GO_P; ++k) if (member[k]) b[k] = 0;
}

void move_go(float *b, int p, int r, int c)
{
    int *l = calculate_liberties(b);                     /* the counts of the board BEFORE the stone is placed */
    if (!l) return;
    b[r * 19 + c] = p;
    remove_group(b, l, -p, r < 18 ? (r + 1) * 19 + c : -1);
    remove_group(b, l, -p, r > 0 ? (r - 1) * 19 + c : -1);
    remove_group(b, l, -p, c < 18 ? r * 19 + c + 1 : -1);
    remove_group(b, l, -p, c > 0 ? r * 19 + c - 1 : -1);
    free(l);
}

static int makes_safe(const float *b, const int *lib, int p, int r, int c)
{
    if (r < 0 || r >= 19 || c < 0 || c >= 19) return 0;
    if (b[r * 19 + c] == -p) return lib[r * 19 + c] <= 1;
    if (b[r * 19 + c] == 0) return 1;
    return lib[r * 19 + c] > 1;
}

int suicide_go(float *b, int p, int r, int c)
{
    int *l = calculate_liberties(b), safe;
    if (!l) return 0;
    safe = makes_safe(b, l, p, r + 1, c) || makes_safe(b, l, p, r - 1, c) || makes_safe(b, l, p, r, c + 1) || makes_safe(b, l, p, r, c - 1);
    free(l);
    return !safe;
}

int legal_go(float *b, char *ko, int p, int r, int c)
{
    char curr[GO_KO], next[GO_KO];
    if (b[r * 19 + c]) return 0;
    board_to_string(curr, b);
    move_go(b, p, r, c);
    board_to_string(next, b);
    string_to_board(curr, b);                            /* the reference's way back: a value other than 0, 1, -1 does not survive it */
    return memcmp(next, ko, GO_KO) != 0;
}

void print_board(float *board, int swap, int *indexes)
{
    FILE *stream = stderr;
    int i, j, n;
    fprintf(stream, "\n\n   ");
    for (i = 0; i < 19; ++i) fprintf(stream, "%c ", 'A' + i + 1 * (i > 7));     /* no I column (noi = 1) */
    fprintf(stream, "\n");
    for (j = 0; j < 19; ++j) {
        fprintf(stream, "%2d", 19 - j);                  /* inverted = 1 */
        for (i = 0; i < 19; ++i) {
            const int index = j * 19 + i;
            int found = 0;
            for (n = 0; indexes && n < 5; ++n) if (index == indexes[n]) { found = 1; fprintf(stream, " %d", n + 1); }
            if (found) continue;
            if (board[index] * -swap > 0) fprintf(stream, " O");
            else if (board[index] * -swap < 0) fprintf(stream, " X");
            else fprintf(stream, "  ");
        }
        fprintf(stream, "\n");
    }
}

/* go.c:21-54: the file is a sequence of 94-byte lines -- the 93-byte record (row, column, 91 packed bytes) and the newline
 * self_go prints behind it; a short tail is dropped.  The library prints nothing (the reference prints the count). */
moves load_go_moves(char *filename)
{
    moves m = { 0, 0 };
    int cap = 128;
    FILE *fp = fopen(filename, "rb");
    if (!fp) { y2_fail("Couldn't open file: %s", filename); return m; }
    m.data = calloc(cap, sizeof(char *));
    for (;;) {
        char *line = malloc(GO_LINE);
        if (fread(line, 1, GO_LINE, fp) != GO_LINE) { free(line); break; }
        if (m.n >= cap) { cap *= 2; m.data = realloc(m.data, cap * sizeof(char *)); }
        m.data[m.n++] = line;
    }
    fclose(fp);
    return m;
}

void y2_go_free_moves(moves m)
{
    int i;
    for (i = 0; i < m.n; ++i) free(m.data[i]);
    free(m.data);
}

int y2_go_draw_moves(int n_records, int batch, int *pick, int *flip, int *rot)
{
    int i;
    if (n_records <= 0) { y2_fail("y2_go_draw_moves: n_records = %d", n_records); return -1; }
    if (batch <= 0 || !pick || !flip || !rot) { y2_fail("y2_go_draw_moves: batch = %d (or a NULL array)", batch); return -1; }
    for (i = 0; i < batch; ++i) {                        /* random_go_moves' three draws per item, in its order */
        pick[i] = rand() % n_records;
        flip[i] = rand() % 2;
        rot[i] = rand() % 4;
    }
    return 0;
}

/* ------------------------------------------------------------------ */
/* refusals: all of them read host memory only                         */
/* ------------------------------------------------------------------ */
static y2_engine *go_engine(const char *who, network *net)
{
    y2_engine *e = y2_engine_of(net);
    if (!e || !net->layers) y2_fail("%s: net: network has no engine (was it built by parse_network_cfg?)", who);
    return net->layers ? e : NULL;
}

static y2_engine *go_net(const char *who, network *net)
{
    y2_engine *e = go_engine(who, net);
    int outputs;
    if (!e) return NULL;
    if (net->w != 19 || net->h != 19 || net->c != 1) {
        y2_fail("%s: net: the network reads %d x %d x %d, a Go network reads 19 x 19 x 1", who, net->w, net->h, net->c);
        return NULL;
    }
    outputs = get_network_output_size(*net);
    if (outputs != GO_P) { y2_fail("%s: net: the network gives %d values, a Go network gives 361", who, outputs); return NULL; }
    if (e->half && !e->strict) {
        y2_fail("%s: net: fp16 mode (y2_set_half / Y2_FP16): Go decisions are compared bit for bit and the half path has no oracle", who);
        return NULL;
    }
    return e;
}

static int go_check_n(const char *who, const char *name, int n)
{
    if (n <= 0) { y2_fail("%s: %s = %d: must be positive", who, name, n); return -1; }
    return 0;
}

static int go_check_boards(const char *who, const float *boards, int n)
{
    size_t i;
    if (!boards) { y2_fail("%s: boards is NULL", who); return -1; }
    for (i = 0; i < (size_t)n * GO_P; ++i)
        if (!(boards[i] == 0 || boards[i] == 1 || boards[i] == -1)) {
            y2_fail("%s: boards: board %d holds %g at point %d; a board holds 0, 1 or -1 (legal_go's string round trip would erase anything else)",
                    who, (int)(i / GO_P), boards[i], (int)(i % GO_P));
            return -1;
        }
    return 0;
}

static int go_check_players(const char *who, const int *players, int n)
{
    int i;
    if (!players) { y2_fail("%s: players is NULL", who); return -1; }
    for (i = 0; i < n; ++i)
        if (players[i] != 1 && players[i] != -1) { y2_fail("%s: players: player %d of position %d; a player is 1 or -1", who, players[i], i); return -1; }
    return 0;
}

/* ------------------------------------------------------------------ */
/* device state: one grow-only HBM block and one pinned block, carved per call */
/* ------------------------------------------------------------------ */
typedef struct y2_go_state {
    unsigned char *d, *h;
    size_t d_cap, h_cap;
    int poll;
} y2_go_state;

void y2_go_free_engine(y2_engine *e)
{
    if (!e->go) return;
    y2h_free(e->go->d); y2h_host_free(e->go->h);
    free(e->go);
    e->go = NULL;
}

static y2_go_state *go_state(y2_engine *e, size_t d_bytes, size_t h_bytes)
{
    y2_go_state *g = e->go;
    if (!g) {
        if (!(g = e->go = calloc(1, sizeof *g))) { y2_fail("go: out of memory"); return NULL; }
        g->poll = 16;      /* measured (profiles/go_stage.txt): games end long before the cap, and asking pays 2.3 - 4.7x */
    }
    if (d_bytes > g->d_cap) {
        y2h_free(g->d); g->d = NULL; g->d_cap = 0;
        if (y2h_malloc((void **)&g->d, d_bytes) != 0) { y2_fail("go: %zu bytes of device memory: %s", d_bytes, y2h_last_error()); return NULL; }
        g->d_cap = d_bytes;
    }
    if (h_bytes > g->h_cap) {
        y2h_host_free(g->h); g->h = NULL; g->h_cap = 0;
        if (y2h_host_alloc((void **)&g->h, h_bytes) != 0) { y2_fail("go: %zu bytes of pinned memory: %s", h_bytes, y2h_last_error()); return NULL; }
        g->h_cap = h_bytes;
    }
    return g;
}

static size_t carve(size_t *off, size_t bytes)
{
    const size_t at = *off;
    *off = at + align_up(bytes ? bytes : 1, 256);
    return at;
}

/* scratch of the forward over n positions: the views and the softmax rows, only when they do not fit one batch */
static size_t go_forward_bytes(const network *net, int n, int multi)
{
    const size_t rows = (size_t)n * (multi ? 8 : 1), padded = (rows + net->batch - 1) / net->batch * net->batch;
    return rows <= (size_t)net->batch ? 0 : 2 * align_up(padded * GO_P * sizeof(float), 256);
}

/* views -> forward -> merge on the network's stream: d_moves[n][361] from d_boards and d_players; `scratch` holds
 * go_forward_bytes.  Rows are processed net.batch at a time. */
static int go_forward(network *net, const float *d_boards, const int *d_players, int n, int multi, float *d_moves, unsigned char *scratch)
{
    y2_engine *e = y2_engine_of(net);
    const size_t rows = (size_t)n * (multi ? 8 : 1), B = net->batch, row = GO_P * sizeof(float);
    const float *out;
    if (rows <= B) {
        HIP_OR_ERR(y2h_go_views(d_boards, d_players, n, multi, e->d_in_nchw, e->stream));
        if (y2_engine_forward(net, e->d_in_nchw) != 0 || y2_output_device(net, &out) != 0) return -1;
        HIP_OR_ERR(y2h_go_merge(out, GO_P, d_boards, n, multi, d_moves, e->stream));
    } else {
        const size_t padded = (rows + B - 1) / B * B;
        float *x = (float *)scratch, *y = (float *)(scratch + align_up(padded * row, 256));
        size_t at;
        HIP_OR_ERR(y2h_memset(x + rows * GO_P, 0, (padded - rows) * row, e->stream));     /* the last chunk's idle rows */
        HIP_OR_ERR(y2h_go_views(d_boards, d_players, n, multi, x, e->stream));
        for (at = 0; at < rows; at += B) {
            HIP_OR_ERR(y2h_memcpy_d2d(e->d_in_nchw, x + at * GO_P, B * row, e->stream));
            if (y2_engine_forward(net, e->d_in_nchw) != 0 || y2_output_device(net, &out) != 0) return -1;
            HIP_OR_ERR(y2h_memcpy_d2d(y + at * GO_P, out, B * row, e->stream));
        }
        HIP_OR_ERR(y2h_go_merge(y, GO_P, d_boards, n, multi, d_moves, e->stream));
    }
    return 0;
}

static void set_temperature(network *net, float temp)
{
    int i;
    for (i = 0; i < net->n; ++i) net->layers[i].temperature = temp;     /* go.c:354 */
}

/* ------------------------------------------------------------------ */
/* batched entries                                                     */
/* ------------------------------------------------------------------ */
int y2_go_predict(network net, const float *boards, const int *players, int n, int multi, float *moves_out)
{
    static const char who[] = "y2_go_predict";
    y2_engine *e = go_net(who, &net);
    y2_go_state *g;
    size_t off = 0, o_b, o_p, o_m, o_s, up;
    if (!e) return -1;
    if (go_check_n(who, "n", n) != 0 || go_check_boards(who, boards, n) != 0 || go_check_players(who, players, n) != 0) return -1;
    if (!moves_out) { y2_fail("%s: moves is NULL", who); return -1; }
    if (y2_prepare(&net) != 0) return -1;
    o_b = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_p = carve(&off, (size_t)n * sizeof(int));
    up = off;
    o_m = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_s = carve(&off, go_forward_bytes(&net, n, multi));
    if (!(g = go_state(e, off, up))) return -1;
    memcpy(g->h + o_b, boards, (size_t)n * GO_P * sizeof(float));
    memcpy(g->h + o_p, players, (size_t)n * sizeof(int));
    HIP_OR_ERR(y2h_memcpy_h2d(g->d, g->h, up, e->stream));
    if (go_forward(&net, (float *)(g->d + o_b), (int *)(g->d + o_p), n, multi, (float *)(g->d + o_m), g->d + o_s) != 0) return -1;
    HIP_OR_ERR(y2h_memcpy_d2h(moves_out, g->d + o_m, (size_t)n * GO_P * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_go_rules(network net, const float *boards, const char *ko, const int *players, int n, int *liberties, unsigned char *legal,
                unsigned char *suicide)
{
    static const char who[] = "y2_go_rules";
    y2_engine *e = go_engine(who, &net);
    y2_go_state *g;
    size_t off = 0, o_b, o_k, o_p, o_l, o_g, o_s, up;
    if (!e) return -1;
    if (go_check_n(who, "n", n) != 0 || go_check_boards(who, boards, n) != 0 || go_check_players(who, players, n) != 0) return -1;
    if (!ko) { y2_fail("%s: ko is NULL (pass n zeroed strings of 91 bytes for none)", who); return -1; }
    HIP_OR_ERR(y2h_set_device(e->device));
    if (!e->stream) HIP_OR_ERR(y2h_stream_create(&e->stream));
    o_b = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_k = carve(&off, (size_t)n * GO_KO);
    o_p = carve(&off, (size_t)n * sizeof(int));
    up = off;
    o_l = carve(&off, (size_t)n * GO_P * sizeof(int));
    o_g = carve(&off, (size_t)n * GO_P);
    o_s = carve(&off, (size_t)n * GO_P);
    if (!(g = go_state(e, off, up))) return -1;
    memcpy(g->h + o_b, boards, (size_t)n * GO_P * sizeof(float));
    memcpy(g->h + o_k, ko, (size_t)n * GO_KO);
    memcpy(g->h + o_p, players, (size_t)n * sizeof(int));
    HIP_OR_ERR(y2h_memcpy_h2d(g->d, g->h, up, e->stream));
    HIP_OR_ERR(y2h_go_rules((float *)(g->d + o_b), g->d + o_k, (int *)(g->d + o_p), n, liberties ? (int *)(g->d + o_l) : NULL,
                            legal ? g->d + o_g : NULL, suicide ? g->d + o_s : NULL, e->stream));
    if (liberties) HIP_OR_ERR(y2h_memcpy_d2h(liberties, g->d + o_l, (size_t)n * GO_P * sizeof(int), e->stream));
    if (legal) HIP_OR_ERR(y2h_memcpy_d2h(legal, g->d + o_g, (size_t)n * GO_P, e->stream));
    if (suicide) HIP_OR_ERR(y2h_memcpy_d2h(suicide, g->d + o_s, (size_t)n * GO_P, e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_go_generate(network net, const float *boards, const char *ko, const int *players, int n, int multi, float thresh, float temp,
                   const float *uniforms, int *index, float *kept)
{
    static const char who[] = "y2_go_generate";
    y2_engine *e = go_net(who, &net);
    y2_go_state *g;
    size_t off = 0, o_b, o_k, o_p, o_u, o_m, o_g, o_s, o_i, o_t, o_f, up;
    if (!e) return -1;
    if (go_check_n(who, "n", n) != 0 || go_check_boards(who, boards, n) != 0 || go_check_players(who, players, n) != 0) return -1;
    if (!ko) { y2_fail("%s: ko is NULL (pass n zeroed strings of 91 bytes for none)", who); return -1; }
    if (!uniforms || !index) { y2_fail("%s: uniforms or index is NULL", who); return -1; }
    set_temperature(&net, temp);
    if (y2_prepare(&net) != 0) return -1;
    o_b = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_k = carve(&off, (size_t)n * GO_KO);
    o_p = carve(&off, (size_t)n * sizeof(int));
    o_u = carve(&off, (size_t)n * sizeof(float));
    up = off;
    o_m = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_g = carve(&off, (size_t)n * GO_P);
    o_s = carve(&off, (size_t)n * GO_P);
    o_i = carve(&off, (size_t)n * sizeof(int));
    o_t = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_f = carve(&off, go_forward_bytes(&net, n, multi));
    if (!(g = go_state(e, off, up))) return -1;
    memcpy(g->h + o_b, boards, (size_t)n * GO_P * sizeof(float));
    memcpy(g->h + o_k, ko, (size_t)n * GO_KO);
    memcpy(g->h + o_p, players, (size_t)n * sizeof(int));
    memcpy(g->h + o_u, uniforms, (size_t)n * sizeof(float));
    HIP_OR_ERR(y2h_memcpy_h2d(g->d, g->h, up, e->stream));
    if (go_forward(&net, (float *)(g->d + o_b), (int *)(g->d + o_p), n, multi, (float *)(g->d + o_m), g->d + o_f) != 0) return -1;
    HIP_OR_ERR(y2h_go_rules((float *)(g->d + o_b), g->d + o_k, (int *)(g->d + o_p), n, NULL, g->d + o_g, g->d + o_s, e->stream));
    HIP_OR_ERR(y2h_go_pick((float *)(g->d + o_m), GO_P, g->d + o_g, g->d + o_s, n, thresh, (float *)(g->d + o_u), (int *)(g->d + o_i),
                           kept ? (float *)(g->d + o_t) : NULL, e->stream));
    HIP_OR_ERR(y2h_memcpy_d2h(index, g->d + o_i, (size_t)n * sizeof(int), e->stream));
    if (kept) HIP_OR_ERR(y2h_memcpy_d2h(kept, g->d + o_t, (size_t)n * GO_P * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_go_valid(network net, const unsigned char *records, int n, int multi, int *predicted)
{
    static const char who[] = "y2_go_valid";
    y2_engine *e = go_net(who, &net);
    y2_go_state *g;
    size_t off = 0, o_r, o_p, o_b, o_m, o_i, o_f, up;
    int i;
    if (!e) return -1;
    if (go_check_n(who, "n", n) != 0) return -1;
    if (!records || !predicted) { y2_fail("%s: records or predicted is NULL", who); return -1; }
    if (y2_prepare(&net) != 0) return -1;
    o_r = carve(&off, (size_t)n * GO_REC);
    o_p = carve(&off, (size_t)n * sizeof(int));
    up = off;
    o_b = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_m = carve(&off, (size_t)n * GO_P * sizeof(float));
    o_i = carve(&off, (size_t)n * sizeof(int));
    o_f = carve(&off, go_forward_bytes(&net, n, multi));
    if (!(g = go_state(e, off, up))) return -1;
    memcpy(g->h + o_r, records, (size_t)n * GO_REC);
    for (i = 0; i < n; ++i) ((int *)(g->h + o_p))[i] = 1;       /* a record's board is the mover's: no flip */
    HIP_OR_ERR(y2h_memcpy_h2d(g->d, g->h, up, e->stream));
    HIP_OR_ERR(y2h_go_decode(g->d + o_r, NULL, NULL, NULL, n, (float *)(g->d + o_b), NULL, e->stream));
    if (go_forward(&net, (float *)(g->d + o_b), (int *)(g->d + o_p), n, multi, (float *)(g->d + o_m), g->d + o_f) != 0) return -1;
    HIP_OR_ERR(y2h_go_argmax((float *)(g->d + o_m), GO_P, n, (int *)(g->d + o_i), e->stream));
    HIP_OR_ERR(y2h_memcpy_d2h(predicted, g->d + o_i, (size_t)n * sizeof(int), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_go_set_poll(network net, int every)
{
    y2_engine *e = go_engine("y2_go_set_poll", &net);
    if (!e) return -1;
    if (every < 0) { y2_fail("y2_go_set_poll: every = %d", every); return -1; }
    if (!go_state(e, 0, 0)) return -1;
    e->go->poll = every;
    return 0;
}

/* self_go's loop (go.c:775-823) for `games` games in lockstep from empty boards.  The reference keeps its two ko strings
 * across games (it never clears `one` / `two` when a game ends); a call here starts every game from zeroed strings, which is
 * what the reference's first game sees. */
int y2_go_selfplay(network net, network net2, int games, int first, int max_moves, int multi, float thresh, float temp,
                   const float *uniforms, unsigned char *records, int *counts, float *final_boards)
{
    static const char who[] = "y2_go_selfplay";
    y2_engine *e = go_net(who, &net), *e2;
    y2_go_state *g;
    size_t off = 0, o_u, o_pl, o_b, o_k, o_a, o_c, o_r, o_m, o_g, o_s, o_i, o_f, up, fb, fb2;
    int t, i, two;
    if (!e) return -1;
    if (!(e2 = go_net(who, &net2))) return -1;
    two = e2 != e;
    if (go_check_n(who, "games", games) != 0 || go_check_n(who, "max_moves", max_moves) != 0) return -1;
    if (first != 0 && first != 1) { y2_fail("%s: first = %d: 0 (net moves first) or 1 (net2 does)", who, first); return -1; }
    if (!uniforms || !records || !counts) { y2_fail("%s: uniforms, records or counts is NULL", who); return -1; }
    if (two && e2->device != e->device) { y2_fail("%s: net2 lives on device %d, net on device %d", who, e2->device, e->device); return -1; }
    set_temperature(&net, temp);
    if (two) set_temperature(&net2, temp);
    if (y2_prepare(&net) != 0 || (two && y2_prepare(&net2) != 0)) return -1;
    o_u = carve(&off, (size_t)games * max_moves * sizeof(float));       /* [max_moves][games]: ply-major for the pick kernel */
    o_pl = carve(&off, (size_t)2 * games * sizeof(int));                /* [games] of +1, then [games] of -1 */
    up = off;
    o_b = carve(&off, (size_t)games * GO_P * sizeof(float));
    o_k = carve(&off, (size_t)2 * games * GO_KO);                       /* the `one` / `two` swap: ply t reads and then writes string t & 1 */
    o_a = carve(&off, (size_t)games * sizeof(int));
    o_c = carve(&off, (size_t)games * sizeof(int));
    o_r = carve(&off, (size_t)games * max_moves * GO_REC);
    o_m = carve(&off, (size_t)games * GO_P * sizeof(float));
    o_g = carve(&off, (size_t)games * GO_P);
    o_s = carve(&off, (size_t)games * GO_P);
    o_i = carve(&off, (size_t)games * sizeof(int));
    fb = go_forward_bytes(&net, games, multi); fb2 = go_forward_bytes(&net2, games, multi);
    o_f = carve(&off, fb > fb2 ? fb : fb2);
    if (!(g = go_state(e, off, up > (size_t)games * sizeof(int) ? up : (size_t)games * sizeof(int)))) return -1;
    for (t = 0; t < max_moves; ++t)
        for (i = 0; i < games; ++i) ((float *)(g->h + o_u))[(size_t)t * games + i] = uniforms[(size_t)i * max_moves + t];
    for (i = 0; i < games; ++i) { ((int *)(g->h + o_pl))[i] = 1; ((int *)(g->h + o_pl))[games + i] = -1; }
    HIP_OR_ERR(y2h_memcpy_h2d(g->d, g->h, up, e->stream));
    HIP_OR_ERR(y2h_memset(g->d + o_b, 0, o_a - o_b, e->stream));        /* empty boards, zeroed ko strings */
    HIP_OR_ERR(y2h_memset(g->d + o_a, 1, (size_t)games * sizeof(int), e->stream));      /* alive: any non-zero value */
    HIP_OR_ERR(y2h_memset(g->d + o_c, 0, o_m - o_c, e->stream));        /* counts and records */
    if (two) HIP_OR_ERR(y2h_stream_sync(e->stream));
    for (t = 0; t < max_moves; ++t) {
        const int player = (t & 1) ? -1 : 1;
        network *use = ((t & 1) == 0) == (first == 0) ? &net : &net2;   /* go.c:799 */
        y2_engine *eu = y2_engine_of(use);
        unsigned char *ko = g->d + o_k + (size_t)(t & 1) * games * GO_KO;
        const int *pl = (int *)(g->d + o_pl) + (player < 0 ? games : 0);
        if (go_forward(use, (float *)(g->d + o_b), pl, games, multi, (float *)(g->d + o_m), g->d + o_f) != 0) return -1;
        HIP_OR_ERR(y2h_go_rules((float *)(g->d + o_b), ko, pl, games, NULL, g->d + o_g, g->d + o_s, eu->stream));
        HIP_OR_ERR(y2h_go_pick((float *)(g->d + o_m), GO_P, g->d + o_g, g->d + o_s, games, thresh,
                               (float *)(g->d + o_u) + (size_t)t * games, (int *)(g->d + o_i), NULL, eu->stream));
        HIP_OR_ERR(y2h_go_play((float *)(g->d + o_b), ko, player, (int *)(g->d + o_i), (int *)(g->d + o_a), g->d + o_r,
                               (int *)(g->d + o_c), max_moves, games, eu->stream));
        if (two) HIP_OR_ERR(y2h_stream_sync(eu->stream));      /* the next ply runs on the other network's stream */
        if (g->poll && (t + 1) % g->poll == 0 && t + 1 < max_moves) {
            int any = 0;
            HIP_OR_ERR(y2h_memcpy_d2h(g->h, g->d + o_a, (size_t)games * sizeof(int), eu->stream));
            HIP_OR_ERR(y2h_stream_sync(eu->stream));
            for (i = 0; i < games; ++i) any |= ((int *)g->h)[i];
            if (!any) break;
        }
    }
    HIP_OR_ERR(y2h_memcpy_d2h(records, g->d + o_r, (size_t)games * max_moves * GO_REC, e->stream));
    HIP_OR_ERR(y2h_memcpy_d2h(counts, g->d + o_c, (size_t)games * sizeof(int), e->stream));
    if (final_boards) HIP_OR_ERR(y2h_memcpy_d2h(final_boards, g->d + o_b, (size_t)games * GO_P * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* ------------------------------------------------------------------ */
/* go.c's two device entries                                           */
/* ------------------------------------------------------------------ */
void predict_move(network net, float *board, float *move, int multi)
{
    const int player = 1;                                /* the caller has already flipped the board (go.c:357) */
    y2_go_predict(net, board, &player, 1, multi, move);
}

/* top_k (utils.c:179-193) */
static void go_top_k(const float *a, int n, int k, int *index)
{
    int i, j;
    for (j = 0; j < k; ++j) index[j] = -1;
    for (i = 0; i < n; ++i) {
        int curr = i;
        for (j = 0; j < k; ++j)
            if (index[j] < 0 || a[curr] > a[index[j]]) { const int swap = curr; curr = index[j]; index[j] = swap; }
    }
}

int generate_move(network net, int player, float *board, int multi, float thresh, float temp, char *ko, int print)
{
    static const char who[] = "generate_move";
    float u, kept[GO_P];
    int index = -1;
    /* everything y2_go_generate would refuse is refused here first, so that a refused call draws nothing */
    if (!go_net(who, &net) || go_check_boards(who, board, 1) != 0 || go_check_players(who, &player, 1) != 0) return -1;
    if (!ko) { y2_fail("%s: ko is NULL (pass a zeroed string of 91 bytes for none)", who); return -1; }
    u = ((float)rand() / RAND_MAX * (1.f - 0.f)) + 0.f;  /* rand_uniform(0, 1) of sample_array (utils.c:524, :610): one draw per call */
    if (y2_go_generate(net, board, ko, &player, 1, multi, thresh, temp, &u, &index, print ? kept : NULL) != 0) return -1;
    if (print) {                                         /* go.c:384-393: the array as sample_array left it, scaled by 1/sum */
        int indexes[5], i;
        float sum = 0;
        for (i = 0; i < GO_P; ++i) sum += kept[i];
        { const float s = 1. / sum; for (i = 0; i < GO_P; ++i) kept[i] *= s; }
        go_top_k(kept, GO_P, 5, indexes);
        for (i = 0; i < 5; ++i) if (!kept[indexes[i]]) indexes[i] = -1;
        print_board(board, player, indexes);
        for (i = 0; i < 5; ++i) fprintf(stderr, "%d: %f\n", i + 1, indexes[i] >= 0 ? kept[indexes[i]] : 0.f);
    }
    return index;
}
