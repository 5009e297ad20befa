/*
 * oatk_amd/csrc/host/multiplex_host.c -- host side of scg_multiplex (syncasm.c:1090-1302) up to its rewrite of the graph: the spanning-triplet
 * table comes from the device (include/oatk_hip_racov.h: oatk_hip_ra_triplet_scores), what the reference decides from it per unitig is
 * decided here.
 *
 * For every unitig that is alive: no live arc at all marks it 2, live arcs on one side only 0.  Otherwise every (incoming, outgoing) pair of
 * live arcs has a score -- the table's, or .001 without an entry --, every arc the largest score of its pairs, the unitig the largest of
 * all.  A unitig longer than max_n_scm syncmers, one with a live arc onto itself, or one whose largest score stays below min_n_r keeps all
 * its pairs (0).  Any other is threaded (1), and a pair that reaches min_d_f of neither its incoming nor its outgoing arc's best is dropped:
 * `updated` counts those.  The rewrite that follows in the reference (:1309-1472) reads multi_vtx[] and the same scores and stays its own.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oatk_hip_racov.h"
#include "oatk_syncasm.h"
#include "host_internal.h"

static void *mx_malloc(size_t n)
{
    void *p = malloc(n? n : 1);
    if (!p) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
    return p;
}

/* live arcs leaving the oriented vertex v */
static uint64_t mx_live(const oatk_asmg_t *ug, uint64_t v)
{
    uint64_t k, n = 0;
    for (k = 0; k < ug->idx_n[v]; ++k) n += !ug->arc[ug->idx_p[v] + k].del;
    return n;
}

uint64_t oatk_host_multiplex_pairs(const oatk_scg_t *g)
{
    const oatk_asmg_t *ug = g->utg_asmg;
    uint64_t i, n = 0;
    for (i = 0; i < ug->n_vtx; ++i) if (!ug->vtx[i].del) n += mx_live(ug, i << 1 | 1) * mx_live(ug, i << 1);
    return n;
}

void oatk_triplet_table_free(oatk_triplet_table *t)
{
    if (!t) return;
    free(t->l_in); free(t->l_out); free(t->val);
    memset(t, 0, sizeof(*t));
}

int oatk_host_multiplex_decide(const oatk_scg_t *g, const uint64_t *pair_off, const uint64_t *pair_in, const uint64_t *pair_out, const double *score,
                               const uint8_t *have, uint32_t max_n_scm, double min_n_r, double min_d_f, uint8_t *multi_vtx, int *updated, oatk_triplet_table *tab)
{
    const oatk_asmg_t *ug = g->utg_asmg;
    uint64_t i, s, t, k, room = 0;
    double *best_in = 0, *best_out = 0;
    int n_dropped = 0;
    for (i = 0; i < ug->n_vtx; ++i) {
        const uint64_t fwd = i << 1, n_in = ug->vtx[i].del? 0 : mx_live(ug, fwd | 1), n_out = ug->vtx[i].del? 0 : mx_live(ug, fwd);
        if (pair_off[i + 1] - pair_off[i] != n_in * n_out) return -1;
        if (n_in + n_out > room) {
            room = 2 * (n_in + n_out);
            free(best_in); free(best_out);
            best_in = (double *) mx_malloc(8 * room), best_out = (double *) mx_malloc(8 * room);
        }
    }
    if (tab) {
        const uint64_t np = pair_off[ug->n_vtx];
        tab->n = 0, tab->m = np;
        tab->l_in = (uint64_t *) mx_malloc(8 * np), tab->l_out = (uint64_t *) mx_malloc(8 * np), tab->val = (double *) mx_malloc(8 * np);
        for (k = 0; k < np; ++k) if (have[k]) tab->l_in[tab->n] = pair_in[k], tab->l_out[tab->n] = pair_out[k], tab->val[tab->n++] = score[k];
    }
    for (i = 0; i < ug->n_vtx; ++i) {
        const uint64_t fwd = i << 1;
        multi_vtx[i] = 0;
        if (ug->vtx[i].del) continue;
        const uint64_t n_in = mx_live(ug, fwd | 1), n_out = mx_live(ug, fwd);
        if (n_in == 0 && n_out == 0) { multi_vtx[i] = 2; continue; }
        if (n_in == 0 || n_out == 0) continue;
        const double *sc = score + pair_off[i];
        const uint8_t *hv = have + pair_off[i];
        double top = .0;
        int loops = 0;
        for (s = 0; s < n_in; ++s) best_in[s] = .0;
        for (t = 0; t < n_out; ++t) best_out[t] = .0;
        for (s = 0; s < n_in; ++s)
            for (t = 0; t < n_out; ++t) {
                const double x = hv[s * n_out + t]? sc[s * n_out + t] : .001;
                if (!(best_in[s] > x)) best_in[s] = x;                      /* MAX(a, b) = a > b? a : b */
                if (!(best_out[t] > x)) best_out[t] = x;
                if (!(top > x)) top = x;
            }
        for (k = 0; k < ug->idx_n[fwd]; ++k) {
            const oatk_asmg_arc_t *a = &ug->arc[ug->idx_p[fwd] + k];
            if (a->w == fwd && !a->del) loops = 1;
        }
        if (ug->vtx[i].n > max_n_scm || loops || top < min_n_r) continue;
        for (s = 0; s < n_in; ++s)
            for (t = 0; t < n_out; ++t) {
                const double x = hv[s * n_out + t]? sc[s * n_out + t] : .001;
                if (x / best_in[s] < min_d_f && x / best_out[t] < min_d_f) ++n_dropped;
            }
        multi_vtx[i] = 1;
    }
    free(best_in); free(best_out);
    *updated = n_dropped;
    return 0;
}

int oatk_scg_multiplex_plan(oatk_hip_ctx *ctx, const oatk_scg_ra_v *ra_v, const oatk_scg_t *g, unsigned flags, uint32_t max_n_scm, double min_n_r,
                            double min_d_f, uint8_t *multi_vtx, int *updated, oatk_triplet_table *tab)
{
    if (!ctx) return OATK_E_NODEV;
    const oatk_asmg_t *ug = g->utg_asmg;
    const uint64_t cap = oatk_host_multiplex_pairs(g);
    void *keep_g = 0, *keep_a = 0;
    const oatk_racov_graph_t *fg = oatk_host_racov_graph(g, 1, &keep_g);
    const oatk_racov_aln_t *fa = 0;
    uint64_t *pair_off = (uint64_t *) mx_malloc(8 * (ug->n_vtx + 1)), *p_in = (uint64_t *) mx_malloc(8 * cap), *p_out = (uint64_t *) mx_malloc(8 * cap), np = 0;
    double *score = (double *) mx_malloc(8 * cap);
    uint8_t *have = (uint8_t *) mx_malloc(cap);
    int rc = OATK_OK;
    if (!(flags & OATK_RACOV_RESIDENT_ALN) && !(fa = oatk_host_racov_aln(ra_v, UINT64_MAX, &keep_a))) rc = OATK_E_ARG;
    if (rc == OATK_OK) rc = oatk_hip_ra_triplet_scores(ctx, fg, fa, pair_off, cap, &np, p_in, p_out, score, have);
    if (rc == OATK_OK && oatk_host_multiplex_decide(g, pair_off, p_in, p_out, score, have, max_n_scm, min_n_r, min_d_f, multi_vtx, updated, tab)) rc = OATK_E_STATE;
    free(pair_off); free(p_in); free(p_out); free(score); free(have);
    oatk_host_racov_graph_free(keep_g);
    oatk_host_racov_aln_free(keep_a);
    return rc;
}
