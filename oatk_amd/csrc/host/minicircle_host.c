/*
 * oatk_amd/csrc/host/minicircle_host.c -- host side of extract_minicircles_with_anchor (path_finder.c:640-730): the distinct repeat units round the
 * anchor come from the device (include/oatk_hip_racov.h: oatk_hip_ra_minicircle_units), already in path_cmpfunc order with the number of records
 * behind each; their lengths and coverage-weighted lengths (:696-727) are computed here from the unitig graph.
 *
 * oatk_mc_path_stats reads the graph and the paths only -- no device -- so that tests/c/minicircle_core_check.cpp runs it under the sanitizers.
 * Its arithmetic is the reference's type for type: len is 32 bits wide and wraps like the reference's, the closing arc takes cov * ls as an integer
 * product that becomes a double afterwards (:712), every other arc (double) cov * ls (:722).  The library is built with -ffp-contract=off.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "oatk_hip_racov.h"
#include "oatk_syncasm.h"
#include "host_internal.h"

static void *mc_malloc(size_t n)
{
    void *p = malloc(n? n : 1);
    if (!p) { fprintf(stderr, "[E::%s] out of memory\n", __func__); exit(EXIT_FAILURE); }
    return p;
}

void oatk_mc_paths_free(oatk_mc_paths *p)
{
    uint64_t i;
    if (!p) return;
    for (i = 0; i < p->n; ++i) free(p->a[i].v);
    free(p->a);
    memset(p, 0, sizeof(*p));
}

/* asmg_arc1 (graph.h:193-205): the first live arc v -> w */
static const oatk_asmg_arc_t *mc_arc1(const oatk_asmg_t *g, uint64_t v, uint64_t w)
{
    uint64_t i;
    for (i = 0; i < g->idx_n[v]; ++i) {
        const oatk_asmg_arc_t *a = &g->arc[g->idx_p[v] + i];
        if (a->w == w && !a->del) return a;
    }
    return 0;
}

int oatk_mc_path_stats(const oatk_asmg_t *g, oatk_mc_paths *paths)
{
    uint64_t i;
    uint32_t j;
    if (!g || !paths) return OATK_E_ARG;
    /* nothing is written unless every path lies in the graph and closes (the reference asserts the arcs, :708 and :720) */
    for (i = 0; i < paths->n; ++i) {
        const oatk_mc_path *p = &paths->a[i];
        if (p->nv == 0) return OATK_E_ARG;
        for (j = 0; j < p->nv; ++j) if ((p->v[j] >> 1) >= g->n_vtx) return OATK_E_ARG;
        for (j = 0; j < p->nv; ++j) if (!mc_arc1(g, p->v[j? j - 1 : p->nv - 1], p->v[j])) return OATK_E_ARG;
    }
    for (i = 0; i < paths->n; ++i) {
        oatk_mc_path *p = &paths->a[i];
        const uint32_t nv = p->nv, *vt = p->v;
        const oatk_asmg_arc_t *a = mc_arc1(g, vt[nv - 1], vt[0]);
        uint32_t len = (uint32_t) g->vtx[vt[0] >> 1].len, len1, cov = g->vtx[vt[0] >> 1].cov;
        double wlen = (double) cov * len;
        len -= a->ls, wlen -= cov * a->ls;                                  /* circular path */
        for (j = 1; j < nv; ++j) {
            len1 = (uint32_t) g->vtx[vt[j] >> 1].len;
            cov = g->vtx[vt[j] >> 1].cov;
            len += len1;
            wlen += (double) cov * len1;
            a = mc_arc1(g, vt[j - 1], vt[j]);
            len -= a->ls;
            wlen -= (double) cov * a->ls;
        }
        p->len = len, p->wlen = wlen;
    }
    return OATK_OK;
}

static void *mc_fetch(oatk_hip_ctx *ctx, int which, uint64_t *bytes, int *rc)
{
    const void *d = 0;
    void *h;
    *bytes = 0;
    *rc = oatk_hip_buffer(ctx, which, &d, bytes);
    if (*rc) return 0;
    h = mc_malloc(*bytes);
    if (*bytes) *rc = oatk_hip_d2h(ctx, h, d, *bytes);
    if (*rc) { free(h); return 0; }
    return h;
}

int oatk_extract_minicircles(oatk_hip_ctx *ctx, const oatk_scg_ra_v *ra_v, const oatk_scg_t *scg, uint64_t anchor_sid, unsigned flags, oatk_mc_paths *out)
{
    void *keep_a = 0;
    const oatk_racov_aln_t *fa = 0;
    uint64_t n_valid = 0, np = 0, npv = 0, b, i, *off = 0, *cnt = 0;
    uint32_t *v = 0;
    oatk_mc_paths res;
    int rc = OATK_OK;
    if (!ctx) return OATK_E_NODEV;
    if (!scg || !scg->utg_asmg || !out) return OATK_E_ARG;
    memset(&res, 0, sizeof(res));
    if (!(flags & OATK_RACOV_RESIDENT_ALN) && !(fa = oatk_host_racov_aln(ra_v, UINT64_MAX, &keep_a))) rc = OATK_E_ARG;
    if (!rc) rc = oatk_hip_ra_minicircle_units(ctx, fa, anchor_sid, &n_valid, &np, &npv);
    oatk_host_racov_aln_free(keep_a);
    if (!rc) off = (uint64_t *) mc_fetch(ctx, OATK_BUF_MC_PATH_OFF, &b, &rc);
    if (!rc) v = (uint32_t *) mc_fetch(ctx, OATK_BUF_MC_PATH_V, &b, &rc);
    if (!rc) cnt = (uint64_t *) mc_fetch(ctx, OATK_BUF_MC_PATH_CNT, &b, &rc);
    if (!rc) {
        res.n = res.m = np;
        res.a = (oatk_mc_path *) mc_malloc(np * sizeof(oatk_mc_path));
        for (i = 0; i < np; ++i) {
            oatk_mc_path *p = &res.a[i];
            p->nv = (uint32_t) (off[i + 1] - off[i]);
            p->v = (uint32_t *) mc_malloc(4 * (size_t) p->nv);
            memcpy(p->v, v + off[i], 4 * (size_t) p->nv);
            p->len = 0, p->wlen = 0., p->cnt = cnt[i];
        }
        rc = oatk_mc_path_stats(scg->utg_asmg, &res);
    }
    free(off); free(v); free(cnt);
    if (rc) { oatk_mc_paths_free(&res); return rc; }
    *out = res;
    return OATK_OK;
}
