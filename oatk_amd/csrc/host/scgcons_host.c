/*
 * oatk_amd/csrc/host/scgcons_host.c -- scg_consensus (syncasm.c:716-823) as a whole: the consensus text of every unitig and the overlap length of every arc.
 *
 * The positions of a unitig's syncmers come from the pair tables (ovl_host.c: oatk_calc_syncmer_overlap, one table per unitig, kept across its pairs as
 * scg_unitig_consensus keeps its own); the skip loop of :1030-1039 turns them into pieces (syncmer, first position not yet written).  All pieces of all unitigs
 * and arcs go to the device in ONE plan (include/oatk_hip_cons.h: oatk_hip_consensus_strings); what comes back is the text and three graph-sized arrays -- the
 * run-length table stays on the device.  The graph is written only when every sequence was served: any refusal leaves it as it was, for the original routine.
 */
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oatk_hip_cons.h"
#include "oatk_syncasm.h"
#include "host_internal.h"

static void *xmalloc(size_t n)
{
    void *p = malloc(n? n : 1);
    if (!p) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
    return p;
}

/* ---- the plan ---- */
typedef struct {
    uint64_t n_seq, m_seq, n_piece, m_piece;
    uint64_t *seq_off, *piece_v;
    int32_t *piece_beg;
    uint8_t *want;
} plan_t;

static void plan_free(plan_t *p) { free(p->seq_off); free(p->piece_v); free(p->piece_beg); free(p->want); }

static void plan_piece(plan_t *p, uint64_t v, int32_t beg)
{
    if (p->n_piece == p->m_piece) {
        p->m_piece = p->m_piece? p->m_piece << 1 : 1024;
        p->piece_v = (uint64_t *) realloc(p->piece_v, p->m_piece * 8);
        p->piece_beg = (int32_t *) realloc(p->piece_beg, p->m_piece * 4);
        if (!p->piece_v || !p->piece_beg) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
    }
    p->piece_v[p->n_piece] = v, p->piece_beg[p->n_piece++] = beg;
}

/* closes the sequence whose pieces were added since the last call; returns its index */
static uint64_t plan_seq(plan_t *p, int want)
{
    if (p->n_seq + 1 >= p->m_seq) {
        p->m_seq = p->m_seq? p->m_seq << 1 : 1024;
        p->seq_off = (uint64_t *) realloc(p->seq_off, (p->m_seq + 1) * 8);
        p->want = (uint8_t *) realloc(p->want, p->m_seq);
        if (!p->seq_off || !p->want) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
        if (p->n_seq == 0) p->seq_off[0] = 0;
    }
    p->want[p->n_seq] = (uint8_t) want;
    p->seq_off[++p->n_seq] = p->n_piece;
    return p->n_seq - 1;
}

/* scg_unitig_consensus (syncasm.c:1004-1046) up to its calls of scg_syncmer_consensus: `here` is where syncmer i starts on the unitig, `done` where the text
 * written so far ends; a syncmer whose successor still starts inside the written part adds nothing.  Returns 0 when a piece would begin at or behind position k
 * or before position -2^31 (the reference asserts the first; no graph of reads gets there): the caller declines with OATK_E_SPLIT. */
static int plan_unitig(plan_t *p, const oatk_overlap_t *o, const uint64_t *v, uint64_t n, int k)
{
    int64_t here = 0, done = 0;
    oatk_ovl_table_t *tab = n? oatk_ovl_table_new() : NULL;
    int ok = 1;
    for (uint64_t i = 0; i < n && ok; ++i) {
        const int last = i + 1 == n;
        const int64_t next = last? 0 : here + oatk_calc_syncmer_overlap(o, v[i], v[i + 1], tab);
        if (last || next > done) {
            const int64_t beg = done - here;
            if (beg >= k || beg < INT32_MIN) ok = 0;
            else plan_piece(p, v[i], (int32_t) beg), done = here + k;
        }
        here = next;
    }
    if (tab) oatk_ovl_table_destroy(tab);
    return ok;
}

/* ---- utg_avg_cov, average_IQR, quantile (syncasm.c:584-664) ---- */
static int dbl_cmp(const void *a, const void *b)
{
    const double x = *(const double *) a, y = *(const double *) b;
    return (x > y) - (x < y);
}

static double quantile_sorted(const double *a, int n, double q)
{
    if (n == 1) return a[0];
    double ip;
    const double fp = modf(q * (n - 1), &ip);
    const int i = (int) lround(ip);
    if (i == n - 1) return a[i];
    return a[i] + (a[i + 1] - a[i]) * fp;
}

static double average_iqr_sorted(const double *a, int n)
{
    if (n == 0) return 0.;
    double q1 = quantile_sorted(a, n, 0.25), q3 = quantile_sorted(a, n, 0.75), s = 0.;
    const double iqr = q3 - q1;
    int i, n0 = 0;
    q1 -= 1.5 * iqr;
    q3 += 1.5 * iqr;
    for (i = 0; i < n; ++i) if (a[i] >= q1 && a[i] <= q3) ++n0, s += a[i];
    return n0? s / n0 : 0.;
}

/* scm_utg_n (syncasm.h:49): entries of scm_u, sixteen bytes each, that name syncmer s */
static uint64_t scm_utg_n(const oatk_scg_t *g, uint64_t s) { return (uint64_t) ((const char *) g->idx_u[s + 1] - (const char *) g->idx_u[s]) / 16; }

static double utg_avg_cov(const oatk_scg_t *g, const oatk_asmg_vtx_t *s)
{
    if (s->del) return .0;
    const oatk_syncmer_t *scm = g->scm_db->a;
    double *cov = (double *) calloc(s->n? s->n : 1, sizeof(double));
    uint64_t i;
    if (!cov) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
    for (i = 0; i < s->n; ++i)                                             /* single-copy syncmers first */
        if (scm_utg_n(g, s->a[i] >> 1) == 1) cov[i] = scm[s->a[i] >> 1].cov;
    qsort(cov, s->n, sizeof(double), dbl_cmp);
    i = 0;
    while (i < s->n && cov[i] < DBL_EPSILON) ++i;
    if (i == s->n) {                                                       /* none: all syncmers */
        for (i = 0; i < s->n; ++i) cov[i] = scm[s->a[i] >> 1].cov;
        qsort(cov, s->n, sizeof(double), dbl_cmp);
        i = 0;
    }
    const double avg = average_iqr_sorted(cov + i, (int) (s->n - i));
    free(cov);
    return avg;
}

/* asmg_arc (graph.h:179-191): the first arc v -> w, deleted or not */
static oatk_asmg_arc_t *find_arc(const oatk_asmg_t *g, uint64_t v, uint64_t w)
{
    oatk_asmg_arc_t *a = g->arc + g->idx_p[v];
    const uint64_t n = g->idx_n[v];
    for (uint64_t i = 0; i < n; ++i) if (a[i].w == w) return &a[i];
    return NULL;
}

static void *fetch(oatk_hip_ctx *ctx, int which, uint64_t want_bytes, int *rc)
{
    const void *d = 0;
    uint64_t b = 0;
    *rc = oatk_hip_buffer(ctx, which, &d, &b);
    if (*rc) return 0;
    if (b != want_bytes) { *rc = OATK_E_STATE; return 0; }
    void *h = xmalloc(b);
    if (b) *rc = oatk_hip_d2h(ctx, h, d, b);
    if (*rc) { free(h); return 0; }
    return h;
}

#define NO_SEQ UINT64_MAX

/* ---- the two halves around the one device call (host_internal.h): oatk_scg_consensus below and oatk_multi_scg_consensus (multi_host.c) run both ---- */
struct oatk_scgcons_plan {
    plan_t p;
    oatk_cons_plan_t dev;                                                  /* p as the device call takes it */
    uint64_t *arc_seq, *vtx_seq;                                           /* the sequence that gives an arc its length (NO_SEQ: 0) / a unitig its text */
};

void oatk_host_scgcons_plan_free(oatk_scgcons_plan_t *sp)
{
    if (!sp) return;
    plan_free(&sp->p);
    free(sp->arc_seq); free(sp->vtx_seq); free(sp);
}

const oatk_cons_plan_t *oatk_host_scgcons_device_plan(const oatk_scgcons_plan_t *sp) { return &sp->dev; }

/* the plan: unitigs (:739-743), then arcs (:779-807); NULL and a code when the graph cannot be served */
oatk_scgcons_plan_t *oatk_host_scgcons_plan(const oatk_overlap_t *o, const oatk_sr_db_t *sr_db, const oatk_scg_t *g, int *rc_out)
{
    const oatk_asmg_t *u = g->utg_asmg;
    const int k = sr_db->k;
    const uint64_t nv = u->n_vtx, na = u->n_arc;
    uint64_t i;
    int rc = OATK_OK;
    oatk_scgcons_plan_t *sp = (oatk_scgcons_plan_t *) xmalloc(sizeof(*sp));
    memset(sp, 0, sizeof(*sp));
    plan_t *p = &sp->p;
    uint64_t *arc_seq = sp->arc_seq = (uint64_t *) xmalloc(na * 8);
    uint64_t *vtx_seq = sp->vtx_seq = (uint64_t *) xmalloc(nv * 8);
    for (i = 0; i < nv && !rc; ++i) {
        const oatk_asmg_vtx_t *s = &u->vtx[i];
        vtx_seq[i] = NO_SEQ;
        if (s->del) continue;
        if (!plan_unitig(p, o, s->a, s->n, k)) rc = OATK_E_SPLIT;
        else vtx_seq[i] = plan_seq(p, 1);
    }
    for (i = 0; i < na && !rc; ++i) {
        const oatk_asmg_arc_t *a = &u->arc[i];
        arc_seq[i] = NO_SEQ;
        if (a->del || a->comp) continue;
        if (!find_arc(u, a->w ^ 1, a->v ^ 1)) { rc = OATK_E_ARG; break; }  /* (the reference would write through a null pointer, :812) */
        if (a->ln > 0) {                                                   /* the overlapping syncmers' own consensus length */
            const oatk_asmg_vtx_t *s = &u->vtx[a->v >> 1];
            if (a->ln > s->n) { rc = OATK_E_ARG; break; }
            if (!plan_unitig(p, o, (a->v & 1)? s->a : s->a + (s->n - a->ln), a->ln, k)) rc = OATK_E_SPLIT;
            else arc_seq[i] = plan_seq(p, 0);
        } else {                                                           /* the overlap of the two end syncmers */
            const oatk_asmg_vtx_t *s = &u->vtx[a->v >> 1], *t = &u->vtx[a->w >> 1];
            if (s->n == 0 || t->n == 0) { rc = OATK_E_ARG; break; }
            uint64_t z = a->v & 1;
            const uint64_t v = s->a[(s->n - 1) * (!z)] ^ z;
            z = a->w & 1;
            const uint64_t w = t->a[(t->n - 1) * z] ^ z;
            const int l = oatk_calc_syncmer_overlap(o, v, w, NULL);
            if (l < k) plan_piece(p, v, l), arc_seq[i] = plan_seq(p, 0);
        }
    }
    *rc_out = rc;
    if (rc) { oatk_host_scgcons_plan_free(sp); return NULL; }
    const oatk_cons_plan_t dev = {p->n_seq, p->n_piece, p->seq_off, p->piece_v, p->piece_beg, p->want};
    sp->dev = dev;
    return sp;
}

/* after the device call on sp's plan (total, refused: what it returned): the text and three small arrays back from ctx, then vtx.len, vtx.cov, vtx.seq, arc.ls and the
 * GFA lines.  The graph and fo are written only when every sequence was served. */
int oatk_host_scgcons_write(oatk_hip_ctx *ctx, const oatk_scgcons_plan_t *sp, uint64_t total, uint64_t refused, oatk_scg_t *g, int save_seq, FILE *fo)
{
    oatk_asmg_t *u = g->utg_asmg;
    const uint64_t nv = u->n_vtx, na = u->n_arc, n_seq = sp->p.n_seq;
    const uint64_t *arc_seq = sp->arc_seq, *vtx_seq = sp->vtx_seq;
    uint64_t i;
    int rc = refused? OATK_E_SPLIT : OATK_OK;
    char *text = 0;
    uint64_t *off = 0, *len = 0;
    uint8_t *status = 0;
    if (!rc) text = (char *) fetch(ctx, OATK_BUF_CONS_STR, total, &rc);
    if (!rc) off = (uint64_t *) fetch(ctx, OATK_BUF_CONS_STR_OFF, (n_seq + 1) * 8, &rc);
    if (!rc) len = (uint64_t *) fetch(ctx, OATK_BUF_CONS_STR_LEN, n_seq * 8, &rc);
    if (!rc) status = (uint8_t *) fetch(ctx, OATK_BUF_CONS_STR_STATUS, n_seq, &rc);
    for (i = 0; i < n_seq && !rc; ++i) if (status[i] || len[i] == UINT64_MAX) rc = OATK_E_SPLIT;
    for (i = 0; i < nv && !rc; ++i)
        if (vtx_seq[i] != NO_SEQ && off[vtx_seq[i] + 1] - off[vtx_seq[i]] != len[vtx_seq[i]]) rc = OATK_E_STATE;

    /* ---- the graph (from here on nothing fails) ---- */
    if (!rc) {
        for (i = 0; i < na; ++i) u->arc[i].ls = 0;                         /* asmg_clean_consensus, graph.h:283-295 */
        for (i = 0; i < nv; ++i) { free(u->vtx[i].seq); u->vtx[i].seq = 0, u->vtx[i].len = 0; }
        if (fo) fprintf(fo, "H\tVN:Z:1.0\n");
        for (i = 0; i < nv; ++i) {
            oatk_asmg_vtx_t *s = &u->vtx[i];
            if (s->del) continue;
            const int64_t l = (int64_t) len[vtx_seq[i]];
            const char *c_seq = text + off[vtx_seq[i]];
            const double cov = s->cov? s->cov : utg_avg_cov(g, s);
            s->cov = cov;
            s->len = l;
            if (save_seq) {
                s->seq = (char *) xmalloc(l + 1);
                memcpy(s->seq, c_seq, l);
                s->seq[l] = 0;
            }
            if (fo) fprintf(fo, "S\tu%lu\t%.*s\tLN:i:%ld\tKC:i:%ld\tSC:f:%.3f\n", (unsigned long) i, (int) l, c_seq, (long) l, (long) (int64_t) (l * cov), cov);
        }
        for (i = 0; i < na; ++i) {
            oatk_asmg_arc_t *a = &u->arc[i];
            if (a->del || a->comp) continue;
            int64_t l = arc_seq[i] == NO_SEQ? 0 : (int64_t) len[arc_seq[i]];
            if ((uint64_t) l > u->vtx[a->v >> 1].len) l = u->vtx[a->v >> 1].len;      /* :809-810 */
            if ((uint64_t) l > u->vtx[a->w >> 1].len) l = u->vtx[a->w >> 1].len;
            a->ls = l;
            find_arc(u, a->w ^ 1, a->v ^ 1)->ls = l;
            if (fo) {
                fprintf(fo, "L\tu%lu\t%c\tu%lu\t%c\t%ldM\tEC:i:%u\n", (unsigned long) (a->v >> 1), "+-"[a->v & 1], (unsigned long) (a->w >> 1), "+-"[a->w & 1], (long) l, a->cov);
                fprintf(fo, "L\tu%lu\t%c\tu%lu\t%c\t%ldM\tEC:i:%u\n", (unsigned long) (a->w >> 1), "-+"[a->w & 1], (unsigned long) (a->v >> 1), "-+"[a->v & 1], (long) l, a->cov);
            }
        }
    }
    free(text); free(off); free(len); free(status);
    return rc;
}

int oatk_scg_consensus(oatk_hip_ctx *ctx, const oatk_overlap_t *o, const oatk_sr_db_t *sr_db, oatk_scg_t *g, int hoco_seq, int save_seq, FILE *fo)
{
    if (!ctx || !o || !sr_db || !g || !g->utg_asmg || !g->scm_db) return OATK_E_ARG;
    int rc = OATK_OK;
    oatk_scgcons_plan_t *sp = oatk_host_scgcons_plan(o, sr_db, g, &rc);
    if (!sp) return rc;
    uint64_t total = 0, refused = 0;
    rc = oatk_hip_consensus_strings(ctx, &sp->dev, hoco_seq, &total, &refused);      /* one device call */
    if (!rc) rc = oatk_host_scgcons_write(ctx, sp, total, refused, g, save_seq, fo);
    oatk_host_scgcons_plan_free(sp);
    return rc;
}
