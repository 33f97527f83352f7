/*
 * Text generation and scoring with [rnn] / [gru] networks: the reference's rnn.c entry points (read_tokens :39,
 * test_char_rnn :225, valid_char_rnn :379, vec_char_rnn :420) and the y2_rnn_* calls they are written on.
 *
 * The reference runs one network_predict per character: a one-hot row up, the forward, 256 probabilities down, the
 * sample on the CPU.  Here the loop stays on the device: a feeder kernel writes the one-hot rows from a token buffer in
 * HBM, the sampling kernel (y2_recurrent.hip) draws the next character from the output row and moves the 1 of the input
 * row in place, and N characters are a plain chain of launches on the engine's stream with one sync at the end.  The
 * host parses, formats text and keeps the books.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "y2_internal.h"

/* ------------------------------------------------------------------ */
/* device loop                                                         */
/* ------------------------------------------------------------------ */
static int grow(void **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return 0;
    y2h_free(*p); *p = NULL; *cap = 0;
    HIP_OR_ERR(y2h_malloc(p, bytes));
    *cap = bytes;
    return 0;
}

void y2_chargen_free(y2_engine *e)
{
    y2h_free(e->d_gen_tok); y2h_free(e->d_gen_u); y2h_free(e->d_gen_p); y2h_free(e->d_gen_probs);
    e->d_gen_tok = NULL; e->d_gen_u = NULL; e->d_gen_p = NULL; e->d_gen_probs = NULL;
    e->gen_tok_cap = e->gen_u_cap = e->gen_p_cap = e->gen_probs_cap = 0;
}

/* what both loops need of the network: sequences B, steps T per forward, the row sizes, the output rows in HBM */
typedef struct { y2_engine *e; int B, T, inputs, outputs; const float *out; } chargen;

static int chargen_open(network *net, const char *who, int generate, chargen *g)
{
    int i, rec = 0;
    g->e = y2_engine_of(net);
    if (!g->e) { y2_fail("%s: network has no engine (was it built by parse_network_cfg?)", who); return -1; }
    for (i = 0; i < net->n; ++i) rec |= is_recurrent(&net->layers[i]);
    if (!rec) { y2_fail("%s: the network has no recurrent layer ([rnn] / [gru])", who); return -1; }
    if (!y2_flat_input(net)) { y2_fail("%s: the network input is an image, not a row of characters", who); return -1; }
    g->T = net->time_steps > 0 ? net->time_steps : 1;
    if (generate && g->T > 1) {
        y2_fail("%s: time_steps=%d: a sampled character is the next forward's input, so generation needs time_steps=1", who, g->T);
        return -1;
    }
    g->B = net->batch / g->T;
    g->inputs = get_network_input_size(*net);
    g->outputs = get_network_output_size(*net);
    if (g->outputs < g->inputs) {
        y2_fail("%s: outputs < inputs: the network gives %d values per character but reads %d", who, g->outputs, g->inputs);
        return -1;
    }
    return 0;
}

/* the plan, once the arguments have passed: everything above is refused without touching the device */
static int chargen_plan(network *net, const char *who, chargen *g)
{
    if (y2_prepare(net) != 0) return -1;
    if (!y2_is_flat(net, g->e->out_layer)) { y2_fail("%s: the output layer is not a flat row per character", who); return -1; }
    g->out = ld_of(&net->layers[g->e->out_layer])->out;
    return 0;
}

static int check_tokens(const char *who, const int *tok, int steps, const chargen *g)
{
    int t, b;
    for (t = 0; t < steps; ++t)
        for (b = 0; b < g->B; ++b) {
            const int c = tok[(size_t)t * g->B + b];
            if (c < 0 || c >= g->inputs) {
                y2_fail("%s: token %d (step %d, sequence %d) is outside the network's %d inputs", who, c, t, b, g->inputs);
                return -1;
            }
        }
    return 0;
}

int y2_rnn_uniforms(int rseed, int n, float *u)
{
    int i;
    if (n < 0 || (n && !u)) { y2_fail("y2_rnn_uniforms: n = %d", n); return -1; }
    srand(rseed);
    for (i = 0; i < n; ++i) u[i] = ((float)rand() / RAND_MAX * (1.f - 0.f)) + 0.f;       /* rand_uniform(0, 1), utils.c:610 */
    return 0;
}

int y2_rnn_generate(network net, const int *seed, int seed_len, int num, const float *uniforms, int *tokens, float *probs)
{
    chargen g;
    y2_engine *e;
    const int S = seed_len > 0 ? seed_len : 1;          /* an empty seed starts from token 0 (rnn.c:245) */
    size_t row;
    int s, i;
    if (chargen_open(&net, "y2_rnn_generate", 1, &g) != 0) return -1;
    e = g.e;
    if (seed_len < 0 || num < 0 || (seed_len && !seed) || (num && (!uniforms || !tokens))) { y2_fail("y2_rnn_generate: bad arguments"); return -1; }
    if (seed_len && check_tokens("y2_rnn_generate", seed, seed_len, &g) != 0) return -1;
    if (chargen_plan(&net, "y2_rnn_generate", &g) != 0) return -1;
    row = (size_t)g.B * sizeof(int);
    if (grow((void **)&e->d_gen_tok, &e->gen_tok_cap, (size_t)(S + num) * row) != 0) return -1;
    if (grow((void **)&e->d_gen_u, &e->gen_u_cap, (size_t)(num ? num : 1) * g.B * sizeof(float)) != 0) return -1;
    if (probs && grow((void **)&e->d_gen_probs, &e->gen_probs_cap, (size_t)(num ? num : 1) * g.B * g.outputs * sizeof(float)) != 0) return -1;
    if (seed_len) HIP_OR_ERR(y2h_memcpy_h2d(e->d_gen_tok, seed, (size_t)S * row, e->stream));
    else HIP_OR_ERR(y2h_memset(e->d_gen_tok, 0, row, e->stream));
    HIP_OR_ERR(y2h_memcpy_h2d(e->d_gen_u, uniforms, (size_t)num * g.B * sizeof(float), e->stream));
    /* the first S-1 seed characters are predicted (rnn.c:257-263); the last one is the first generating input */
    for (s = 0; s < S; ++s) {
        HIP_OR_ERR(y2h_rnn_feed(e->d_gen_tok + (size_t)s * g.B, e->d_in_nchw, g.B, g.inputs, e->stream));
        if (s < S - 1 && y2_engine_forward(&net, e->d_in_nchw) != 0) return -1;
    }
    for (i = 0; i < num; ++i) {
        int *at = e->d_gen_tok + (size_t)(S - 1 + i) * g.B;
        if (y2_engine_forward(&net, e->d_in_nchw) != 0) return -1;
        HIP_OR_ERR(y2h_rnn_sample(g.out, g.outputs, g.inputs, g.B, e->d_gen_u + (size_t)i * g.B, at, at + g.B, e->d_in_nchw,
                                  probs ? e->d_gen_probs + (size_t)i * g.B * g.outputs : NULL, e->stream));
    }
    HIP_OR_ERR(y2h_memcpy_d2h(tokens, e->d_gen_tok + (size_t)S * g.B, (size_t)num * row, e->stream));
    if (probs) HIP_OR_ERR(y2h_memcpy_d2h(probs, e->d_gen_probs, (size_t)num * g.B * g.outputs * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

int y2_rnn_score(network net, const int *tokens, int n, float *p_next, float *probs)
{
    chargen g;
    y2_engine *e;
    size_t rows;
    int c;
    if (chargen_open(&net, "y2_rnn_score", 0, &g) != 0) return -1;
    e = g.e;
    if (n < 1 || !tokens || (n > 1 && !p_next)) { y2_fail("y2_rnn_score: bad arguments"); return -1; }
    if ((n - 1) % g.T) {
        y2_fail("y2_rnn_score: %d characters to score is not a multiple of time_steps=%d (pass a multiple plus the one that follows)", n - 1, g.T);
        return -1;
    }
    if (check_tokens("y2_rnn_score", tokens, n, &g) != 0) return -1;
    if (chargen_plan(&net, "y2_rnn_score", &g) != 0) return -1;
    rows = (size_t)(n - 1) * g.B;
    if (!rows) return 0;
    if (grow((void **)&e->d_gen_tok, &e->gen_tok_cap, (size_t)n * g.B * sizeof(int)) != 0) return -1;
    if (grow((void **)&e->d_gen_p, &e->gen_p_cap, rows * sizeof(float)) != 0) return -1;
    if (probs && grow((void **)&e->d_gen_probs, &e->gen_probs_cap, rows * g.outputs * sizeof(float)) != 0) return -1;
    HIP_OR_ERR(y2h_memcpy_h2d(e->d_gen_tok, tokens, (size_t)n * g.B * sizeof(int), e->stream));
    for (c = 0; c < (n - 1) / g.T; ++c) {               /* one forward scores T characters of every sequence */
        const size_t r0 = (size_t)c * g.T * g.B;
        HIP_OR_ERR(y2h_rnn_feed(e->d_gen_tok + r0, e->d_in_nchw, g.T * g.B, g.inputs, e->stream));
        if (y2_engine_forward(&net, e->d_in_nchw) != 0) return -1;
        HIP_OR_ERR(y2h_rnn_score(g.out, g.outputs, e->d_gen_tok + r0 + g.B, g.T * g.B, e->d_gen_p + r0,
                                 probs ? e->d_gen_probs + r0 * g.outputs : NULL, e->stream));
    }
    HIP_OR_ERR(y2h_memcpy_d2h(p_next, e->d_gen_p, rows * sizeof(float), e->stream));
    if (probs) HIP_OR_ERR(y2h_memcpy_d2h(probs, e->d_gen_probs, rows * g.outputs * sizeof(float), e->stream));
    HIP_OR_ERR(y2h_stream_sync(e->stream));
    return 0;
}

/* ------------------------------------------------------------------ */
/* bookkeeping                                                         */
/* ------------------------------------------------------------------ */
/* rnn.c:402-414 for one character: `next` followed with probability p */
typedef struct { float sum; int count, words; } perp_books;

static void perp_step(perp_books *k, float p, int next)
{
    const float log2 = log(2);
    ++k->count;
    if (next == ' ' || next == '\n' || next == '\t') ++k->words;
    k->sum += log(p) / log2;
}

int y2_rnn_perplexity(const float *p_next, const unsigned char *text, int n, float *perplexity, float *word_perplexity)
{
    perp_books k = { 0, 0, 1 };
    int i;
    if (n < 2 || !p_next || !text) { y2_fail("y2_rnn_perplexity: needs a text of at least 2 characters"); return -1; }
    for (i = 0; i + 1 < n; ++i) perp_step(&k, p_next[i], text[i + 1]);
    if (perplexity) *perplexity = pow(2, -k.sum / k.count);
    if (word_perplexity) *word_perplexity = pow(2, -k.sum / k.words);
    return 0;
}

/* ------------------------------------------------------------------ */
/* rnn.c entry points                                                  */
/* ------------------------------------------------------------------ */
char **read_tokens(char *filename, size_t *read)          /* rnn.c:39-58 */
{
    size_t size = 512, count = 0;
    FILE *fp = fopen(filename, "r");
    char **d, *line;
    if (read) *read = 0;
    if (!fp) { y2_fail("Couldn't open file: %s", filename); return NULL; }
    d = calloc(size, sizeof(char *));
    while ((line = y2_fgetl(fp)) != 0) {
        if (++count > size) { size *= 2; d = realloc(d, size * sizeof(char *)); }
        d[count - 1] = line;
    }
    fclose(fp);
    if (read) *read = count;
    return d;
}

static network open_net(char *cfgfile, char *weightfile)
{
    network net;
    fprintf(stderr, "%s\n", basecfg(cfgfile));
    net = parse_network_cfg(cfgfile);
    if (net.layers && weightfile) load_weights(&net, weightfile);
    return net;
}

static int print_symbol(int n, char **tokens, size_t n_tokens)     /* rnn.c:217-223 */
{
    if (!tokens) { printf("%c", n); return 0; }
    if (n < 0 || (size_t)n >= n_tokens) { y2_fail("token %d has no line in the token file (%zu lines)", n, n_tokens); return -1; }
    printf("%s ", tokens[n]);
    return 0;
}

/* characters as the one sequence they are in the reference, on each of the B sequences the cfg asks for */
static int *spread(const char *s, int len, int B)
{
    int *t = calloc((size_t)(len ? len : 1) * B, sizeof(int)), i, b;
    for (i = 0; i < len; ++i) for (b = 0; b < B; ++b) t[(size_t)i * B + b] = s[i];     /* `c = seed[i]`: a plain char, rnn.c:258 */
    return t;
}

void test_char_rnn(char *cfgfile, char *weightfile, int num, char *seed, float temp, int rseed, char *token_file)
{
    enum { CHUNK = 256 };
    char **tokens = 0;
    size_t n_tokens = 0;
    network net;
    int i, b, B, len, done, *seedt = NULL, *out = NULL;
    float *u = NULL, *ub = NULL;
    if (token_file && !(tokens = read_tokens(token_file, &n_tokens))) return;
    net = open_net(cfgfile, weightfile);
    if (!net.layers) return;
    for (i = 0; i < net.n; ++i) net.layers[i].temperature = temp;     /* rnn.c:244 */
    B = net.batch;
    len = strlen(seed);
    seedt = spread(seed, len, B);
    u = calloc(num > 0 ? num : 1, sizeof(float));
    ub = calloc((size_t)CHUNK * B, sizeof(float));
    out = calloc((size_t)CHUNK * B, sizeof(int));
    if (y2_rnn_uniforms(rseed, num > 0 ? num : 0, u) != 0) goto done;     /* srand(rseed), one rand_uniform per draw (utils.c:524) */
    for (i = 0; i < (len ? len : 1); ++i) if (print_symbol(seedt[(size_t)i * B], tokens, n_tokens) != 0) goto done;
    for (done = 0; done < num || (done == 0 && len > 1); ) {
        const int n = num - done < CHUNK ? (num - done > 0 ? num - done : 0) : CHUNK;
        for (i = 0; i < n; ++i) for (b = 0; b < B; ++b) ub[(size_t)i * B + b] = u[done + i];
        if (y2_rnn_generate(net, seedt, done ? 1 : len, n, ub, out, NULL) != 0) goto done;
        for (i = 0; i < n; ++i) if (print_symbol(out[(size_t)i * B], tokens, n_tokens) != 0) goto done;
        if (!n) break;
        memcpy(seedt, out + (size_t)(n - 1) * B, (size_t)B * sizeof(int));     /* the next chunk goes on from the last character */
        done += n;
    }
    printf("\n");
done:
    free(seedt); free(u); free(ub); free(out);
    for (i = 0; tokens && (size_t)i < n_tokens; ++i) free(tokens[i]);
    free(tokens);
    free_network(net);
}

void valid_char_rnn(char *cfgfile, char *weightfile, char *seed)
{
    network net = open_net(cfgfile, weightfile);
    const int len = strlen(seed);
    size_t cap = 1 << 16, n = 0;
    unsigned char *text;
    perp_books k = { 0, 0, 1 };
    int c, B, T, chunk, *tok = NULL;
    float *p = NULL;
    size_t at, i;
    if (!net.layers) return;
    T = net.time_steps > 0 ? net.time_steps : 1;
    B = net.batch / T;
    text = malloc(cap);
    for (i = 0; i < (size_t)len; ++i) text[n++] = (unsigned char)seed[i];      /* the seed is predicted, not scored (rnn.c:396-401) */
    while ((c = getc(stdin)) != EOF) {
        if (n > (size_t)len && c >= 255) { y2_fail("Out of range character"); goto done; }    /* rnn.c:408 */
        if (n == cap) text = realloc(text, cap *= 2);
        text[n++] = (unsigned char)c;
    }
    chunk = 1024 * T;
    tok = calloc((size_t)(chunk + 1) * B, sizeof(int));
    p = calloc((size_t)chunk * B, sizeof(float));
    for (at = 0; at + 1 < n; at += chunk) {              /* the state carries on from chunk to chunk */
        const size_t m = n - 1 - at < (size_t)chunk ? n - 1 - at : (size_t)chunk;
        int b;
        for (i = 0; i <= m; ++i) for (b = 0; b < B; ++b) tok[i * B + b] = (len && at + i < (size_t)len) ? seed[at + i] : text[at + i];
        if (y2_rnn_score(net, tok, (int)m + 1, p, NULL) != 0) goto done;
        for (i = 0; i < m; ++i) {
            if (at + i + 1 <= (size_t)len) continue;     /* still inside the seed, or the seed's last character predicting the first of the text */
            perp_step(&k, p[i * B], text[at + i + 1]);
            printf("%d Perplexity: %4.4f    Word Perplexity: %4.4f\n", k.count, pow(2, -k.sum / k.count), pow(2, -k.sum / k.words));
        }
    }
done:
    free(text); free(tok); free(p);
    free_network(net);
}

void vec_char_rnn(char *cfgfile, char *weightfile, char *seed)
{
    network net = open_net(cfgfile, weightfile);
    const int seed_len = strlen(seed);
    char *line;
    int T, B;
    if (!net.layers) return;
    T = net.time_steps > 0 ? net.time_steps : 1;
    B = net.batch / T;
    while ((line = y2_fgetl(stdin)) != 0) {
        const layer *l = &net.layers[0];
        int str_len, n, i, *tok;
        float *v;
        y2_strip(line);
        str_len = strlen(line);
        n = seed_len + str_len + 1;                      /* the seed, the line, a space (rnn.c:438-455) */
        {
            char *all = malloc((size_t)n + 1);
            memcpy(all, seed, seed_len); memcpy(all + seed_len, line, str_len); all[n - 1] = ' '; all[n] = 0;
            tok = spread(all, n, B);
            free(all);
        }
        /* scoring n characters plus any follower runs exactly the n forwards of the reference; the follower is never fed */
        tok = realloc(tok, (size_t)(n + 1) * B * sizeof(int));
        for (i = 0; i < B; ++i) tok[(size_t)n * B + i] = 0;
        {   /* one buffer for the n*B scores (not used) and then layer 0's T*B rows */
            const size_t scores = (size_t)n * B, rows = (size_t)T * B * l->outputs;
            v = calloc(scores > rows ? scores : rows, sizeof(float));
        }
        reset_rnn_state(net, 0);
        if (y2_rnn_score(net, tok, n + 1, v, NULL) != 0 || y2_pull_layer_output(net, 0, v) != 0) { free(tok); free(v); free(line); break; }
        printf("%s", line);
        for (i = 0; i < l->outputs; ++i) printf(",%g", v[(size_t)(T - 1) * B * l->outputs + i]);     /* sequence 0, the last step */
        printf("\n");
        free(tok); free(v); free(line);
    }
    free_network(net);
}
