// pmx_backward.hip -- the head backward of the C ABI: pmx_backward_enable / pmx_backward_head / pmx_get_layer_grad / pmx_get_trunk_grad /
// pmx_get_retained.  Semantics and the orders of every sum: include/pose_mi355x.h; the stores' layout: pmx_ctx.h (BwState); the forward's
// side of retention: pmx_api.hip (pmx_forward_from_in16).  This file holds no kernel: the data gradients are plans of the forward's
// dispatcher on transposed packs (pmx_run_conv), everything else is a launch of conv_bwd.hip.
#include "pmx_ctx.h"

#include <stdio.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int N_LG = PMX_N_PAF + PMX_N_HEAT;      // floats per pixel of a stage's loss gradient (pmx_loss.hip)

bool stage_out(int k) { return k == PMX_BW_S1 + 4 || (k >= PMX_BW_M2 && k < PMX_BW_X42 && (k - PMX_BW_M2) % 7 == 6); }
int slot_stage(int k) { return k < PMX_BW_S1 ? 0 : k < PMX_BW_M2 ? 1 : k < PMX_BW_X42 ? 2 + (k - PMX_BW_M2) / 7 : 0; }

// names, leading dimensions and offsets of the slots, the gradient store's offsets; no allocation
int bw_layout(pmx_ctx* c)
{
    BwState& bw = c->bw;
    bw.cap_px = (size_t)c->max_batch * ((size_t)c->max_h * c->max_w / 64);
    bw.layer_slot.assign(c->table.size(), -1);
    auto put = [&](int k, const char* n1, const char* n2, int lda, int ldg) -> int {
        auto i1 = c->index.find(n1), i2 = c->index.find(n2);
        PMX_CHECK(i1 != c->index.end() && i2 != c->index.end(), PMX_ERR_STATE, "backward: no layer '%s' / '%s'", n1, n2);
        bw.slot_layer[k][0] = i1->second; bw.slot_layer[k][1] = i2->second;
        bw.layer_slot[i1->second] = 2 * k;
        if (i2->second != i1->second) bw.layer_slot[i2->second] = 2 * k + 1;
        bw.slot[k].lda = lda; bw.slot[k].ldg = ldg;
        return PMX_OK;
    };
    int rc;
    char n1[48], n2[48];
    if ((rc = put(PMX_BW_C43, "conv4_3_CPM", "conv4_3_CPM", 256, 256)) || (rc = put(PMX_BW_C44, "conv4_4_CPM", "conv4_4_CPM", 0, 128)) ||
        (rc = put(PMX_BW_X42, "conv4_2", "conv4_2", 512, 0))) return rc;
    for (int i = 1; i <= 5; ++i) {
        snprintf(n1, sizeof n1, "conv5_%d_CPM_L1", i); snprintf(n2, sizeof n2, "conv5_%d_CPM_L2", i);
        if ((rc = put(PMX_BW_S1 + i - 1, n1, n2, i == 4 ? 1024 : i == 5 ? 64 : 256, i == 4 ? 1024 : i == 5 ? 128 : 256))) return rc;
    }
    for (int s = 2; s <= 6; ++s)
        for (int i = 1; i <= 7; ++i) {
            snprintf(n1, sizeof n1, "Mconv%d_stage%d_L1", i, s); snprintf(n2, sizeof n2, "Mconv%d_stage%d_L2", i, s);
            if ((rc = put(PMX_BW_M(s, i), n1, n2, i == 7 ? 64 : 256, i == 7 ? 128 : 256))) return rc;
        }
    bw.layer_slot[c->index.at("conv4_2")] = -1;      // (a trunk layer: a slot for its output, no gradients)
    size_t a = 0, g = 0;
    for (int k = 0; k < PMX_BW_SLOTS; ++k) {         // (every leading dimension is a multiple of 64 floats: the slots stay 256-byte aligned)
        bw.slot[k].a_off = a; bw.slot[k].g_off = g;
        a += bw.cap_px * bw.slot[k].lda; g += bw.cap_px * bw.slot[k].ldg;
    }
    bw.grad_off.assign(c->table.size(), 0);
    size_t off = 0;
    for (size_t i = 0; i < c->table.size(); ++i) {
        if (bw.layer_slot[i] < 0) continue;
        const LayerDesc& d = c->table[i];
        bw.grad_off[i] = off;
        off += ((size_t)d.cout * d.cin * d.ks * d.ks + d.cout + 63) / 64 * 64;
    }
    // a refused allocation is a capacity error of this context's size, not a runtime failure
    DevBuf<float>* const bufs[] = {&bw.act, &bw.g, &bw.grad, &bw.u, &bw.dcat, &bw.fg, &bw.trunk};
    const size_t counts[] = {a, g, off, bw.cap_px * 1024, bw.cap_px * 2 * PMX_CAT_C, bw.cap_px * 128, bw.cap_px * 512};
    bool ok = true;
    for (int i = 0; i < 7 && ok; ++i) ok = bufs[i]->alloc(counts[i]) == PMX_OK;
    ok = ok && bw.part.alloc((size_t)PMX_DB_SLOTS * 1024) == PMX_OK && bw.cat_of_ref.alloc(185) == PMX_OK;
    if (!ok) {
        (void)hipGetLastError();
        pmx_set_error("pmx_backward_enable: the device has no room for the stores of %d x %d x %d (%.2f GB of activations, %.2f GB of gradients)",
                      c->max_batch, c->max_h, c->max_w, a * 4e-9, g * 4e-9);
        return PMX_ERR_CAPACITY;
    }
    // poison: an element the backward fails to write is caught by the tests
    PMX_HIP(hipMemsetAsync(bw.g, 0xFF, g * sizeof(float), c->stream));
    PMX_HIP(hipMemsetAsync(bw.grad, 0xFF, off * sizeof(float), c->stream));
    PMX_HIP(hipMemsetAsync(bw.trunk, 0xFF, bw.cap_px * 512 * sizeof(float), c->stream));
    int map[185];
    for (int i = 0; i < 38; ++i) map[i] = PMX_CAT_PAF + i;
    for (int i = 0; i < 19; ++i) map[38 + i] = PMX_CAT_HEAT + i;
    for (int i = 0; i < 128; ++i) map[57 + i] = PMX_CAT_FEAT + i;
    PMX_HIP(hipMemcpy(bw.cat_of_ref, map, sizeof map, hipMemcpyHostToDevice));
    return PMX_OK;
}

void bw_free(BwState& bw)
{
    bw.act.reset(); bw.g.reset(); bw.grad.reset(); bw.u.reset(); bw.dcat.reset(); bw.fg.reset(); bw.trunk.reset(); bw.ws.reset(); bw.part.reset();
    bw.cat_of_ref.reset();
}

// the checks every entry but pmx_backward_enable shares; need_done: pmx_backward_head must have run for the retained forward
int bw_check(pmx_ctx* c, const char* who, bool need_done)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "%s: null ctx", who);
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "%s: the head backward exists for posenet contexts only", who);
    PMX_CHECK(c->opt_precision == 0, PMX_ERR_STATE, "%s: option \"precision\" is %d; the gradients are fp32 only", who, c->opt_precision);
    PMX_CHECK(c->bw.on && c->bw.valid, PMX_ERR_STATE,
              "%s: no retained forward (pmx_backward_enable, pmx_loss_enable and pmx_loss_grad_enable on, then a uniform fp32 forward; any other "
              "forward since discards it)", who);
    PMX_CHECK(!need_done || c->bw.done, PMX_ERR_STATE, "%s: pmx_backward_head has not run for the retained forward", who);
    return PMX_OK;
}

// slot and branch of a layer of the head that the retained forward ran
int bw_find(pmx_ctx* c, const char* who, const char* name, bool allow_x42, int* slot, int* branch)
{
    PMX_CHECK(name, PMX_ERR_INVALID, "%s: null layer name", who);
    if (allow_x42 && !strcmp(name, "conv4_2")) { *slot = PMX_BW_X42; *branch = 0; return PMX_OK; }
    auto it = c->index.find(name);
    PMX_CHECK(it != c->index.end() && c->bw.layer_slot[it->second] >= 0, PMX_ERR_INVALID, "%s: '%s' is not one of the 82 layers after conv4_2", who, name);
    *slot = c->bw.layer_slot[it->second] / 2; *branch = c->bw.layer_slot[it->second] % 2;
    PMX_CHECK(slot_stage(*slot) <= c->bw.stages, PMX_ERR_STATE, "%s: '%s': the retained forward ran %d stages (option \"stop_stage\")", who, name,
              c->bw.stages);
    return PMX_OK;
}

// NHWC device (C channels from `src`, ld floats per pixel) -> NCHW host
int fetch_nchw(pmx_ctx* c, const float* src, int ld, int C, float* out)
{
    const BwState& bw = c->bw;
    const size_t n = (size_t)bw.B * C * bw.fh * bw.fw;
    DevBuf<float> tmp;
    int rc;
    if ((rc = tmp.alloc(n)) || (rc = launch_nhwc_to_nchw(src, tmp, bw.B, C, bw.fh, bw.fw, ld, 0, c->stream))) return rc;
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(out, tmp, n * sizeof(float), hipMemcpyDeviceToHost));
    return PMX_OK;
}

}  // namespace

extern "C" int pmx_backward_enable(pmx_ctx* c, int on)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "pmx_backward_enable: null ctx");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_backward_enable: the head backward exists for posenet contexts only");
    PMX_DEV(c);
    BwState& bw = c->bw;
    if (!on) {
        if (bw.on) { PMX_HIP(hipStreamSynchronize(c->stream)); pmx_train_free(c); bw_free(bw); }      // (training lives on the gradient store)
        bw.on = 0; bw.valid = bw.done = false;
        return PMX_OK;
    }
    if (bw.on) return PMX_OK;
    if (bw.tl.size() != c->layers.size()) bw.tl.resize(c->layers.size());
    if (int rc = bw_layout(c)) { bw_free(bw); return rc; }
    bw.on = 1; bw.valid = bw.done = false;
    return PMX_OK;
}

extern "C" int pmx_backward_head(pmx_ctx* c)
{
    int rc;
    if ((rc = bw_check(c, "pmx_backward_head", false))) return rc;
    PMX_CHECK(c->lg_on && c->lg_stages == c->bw.stages && c->lg_B == c->bw.B && c->lg_fh == c->bw.fh && c->lg_fw == c->bw.fw, PMX_ERR_STATE,
              "pmx_backward_head: the loss gradients of the retained forward are gone (pmx_loss_grad_enable)");
    PMX_DEV(c);
    BwState& bw = c->bw;
    const int n = bw.stages, B = bw.B, fh = bw.fh, fw = bw.fw;
    const long long npix = (long long)B * fh * fw;
    hipStream_t st = c->stream;
    // before anything is enqueued: the data-gradient packs and the workspace of the widest weight gradient
    size_t ws_need = 0;
    for (int k = 0; k < PMX_BW_X42; ++k) {
        if (slot_stage(k) > n) continue;
        for (int b = 0; b < 2; ++b) {
            const int idx = bw.slot_layer[k][b];
            if ((rc = pmx_bw_transposed_pack(c, idx))) return rc;
            const LayerDesc& d = c->table[idx];
            const int cg = round_up(d.cout, 32), cx = round_up(d.cin, 32);
            int rows = 0;
            const int strips = conv_wgrad_strips(B, fh, cg, cx, d.ks, c->opt_wgrad_strips, &rows);
            ws_need = std::max(ws_need, (size_t)strips * d.ks * d.ks * cg * cx);
        }
    }
    if ((rc = bw.ws.ensure(ws_need, st))) return rc;

    auto A = [&](int k) { return bw.act + bw.slot[k].a_off; };
    auto G = [&](int k) { return bw.g + bw.slot[k].g_off; };
    // db and dw of one layer from its g and its input x (both slices: ldg / ldx floats per pixel)
    auto grads = [&](int idx, const float* g, int ldg, const float* x, int ldx) -> int {
        const LayerDesc& d = c->table[idx];
        const int cg = round_up(d.cout, 32), cx = round_up(d.cin, 32);
        float* dw = bw.grad + bw.grad_off[idx];
        float* db = dw + (size_t)d.cout * d.cin * d.ks * d.ks;
        int rows = 0;
        const int strips = conv_wgrad_strips(B, fh, cg, cx, d.ks, c->opt_wgrad_strips, &rows);
        if (int r = conv_bwd_db_launch(g, ldg, bw.part, db, npix, d.cout, cg, st)) return r;
        return conv_wgrad_launch(g, ldg, x, ldx, bw.ws, dw, B, fh, fw, d.cout, cg, d.cin, cx, d.ks, strips, rows,
                                 d.cin == 185 ? bw.cat_of_ref.get() : nullptr, st);
    };
    // both branches of slot k: g at G(k) and G(k) + goff, x at x0 and x1
    auto grads2 = [&](int k, int goff, const float* x0, const float* x1, int ldx) -> int {
        const int ldg = bw.slot[k].ldg;
        if (int r = grads(bw.slot_layer[k][0], G(k), ldg, x0, ldx)) return r;
        return grads(bw.slot_layer[k][1], G(k) + goff, ldg, x1, ldx);
    };
    // the data gradient of slot k's layer pair (one layer: o1 null) through the dispatcher
    auto dgrad = [&](int k, int goff, float* o0, float* o1, int ldc) -> int {
        const int i0 = bw.slot_layer[k][0], i1 = bw.slot_layer[k][1];
        char label[64];
        snprintf(label, sizeof label, "bwd_dx:%s", c->table[i0].name.c_str());
        return pmx_run_conv(c, label, &bw.tl[i0], o1 ? &bw.tl[i1] : nullptr, G(k), o1 ? G(k) + goff : nullptr, bw.slot[k].ldg, o0, o1, ldc, B, fh, fw, 0);
    };
    auto mask = [&](const float* u, int ldu, const float* a, int lda, int k) -> int {
        return bwd_mask_nhwc_launch(u, ldu, a, lda, G(k), bw.slot[k].ldg, npix, bw.slot[k].ldg, st);
    };
    float* const u = bw.u;
    float* const dcat = bw.dcat;
    float* const cat = c->cat;
    const float* lg = c->ls_grad;
#define BW(x) do { if ((rc = (x))) return rc; } while (0)
    for (int s = n; s >= 2; --s) {
        const int k7 = PMX_BW_M(s, 7), prev = s == 2 ? PMX_BW_S1 + 4 : PMX_BW_M(s - 1, 7);
        BW(bwd_stage_sum_launch(lg + (size_t)(s - 1) * npix * N_LG, s == n ? nullptr : dcat, s == n ? nullptr : dcat + PMX_CAT_C, 2 * PMX_CAT_C, G(k7), npix, st));
        BW(grads2(k7, 64, A(PMX_BW_M(s, 6)), A(PMX_BW_M(s, 6)) + 128, 256));
        BW(dgrad(k7, 64, u, u + 128, 256));
        for (int i = 6; i >= 1; --i) {
            const int k = PMX_BW_M(s, i);
            BW(mask(u, 256, A(k), 256, k));
            if (i > 1) {
                BW(grads2(k, 128, A(PMX_BW_M(s, i - 1)), A(PMX_BW_M(s, i - 1)) + 128, 256));
                BW(dgrad(k, 128, u, u + 128, 256));
            } else {
                // Mconv1 read the concat buffer as stage s - 1 left it
                BW(bwd_copy_cols_launch(A(prev), 64, cat + PMX_CAT_PAF, PMX_CAT_C, npix, 64, st));
                BW(grads2(k, 128, cat, cat, PMX_CAT_C));
                BW(dgrad(k, 128, dcat, dcat + PMX_CAT_C, 2 * PMX_CAT_C));
                BW(bwd_feat_sum_launch(bw.fg, dcat + PMX_CAT_FEAT, dcat + PMX_CAT_C + PMX_CAT_FEAT, 2 * PMX_CAT_C, s == n, npix, st));
            }
        }
    }
    {   // stage 1
        const int k5 = PMX_BW_S1 + 4, k4 = PMX_BW_S1 + 3;
        BW(bwd_stage_sum_launch(lg, n == 1 ? nullptr : dcat, n == 1 ? nullptr : dcat + PMX_CAT_C, 2 * PMX_CAT_C, G(k5), npix, st));
        BW(grads2(k5, 64, A(k4), A(k4) + 512, 1024));
        BW(dgrad(k5, 64, u, u + 512, 1024));
        BW(mask(u, 1024, A(k4), 1024, k4));
        BW(grads2(k4, 512, A(PMX_BW_S1 + 2), A(PMX_BW_S1 + 2) + 128, 256));
        BW(dgrad(k4, 512, u, u + 128, 256));
        for (int i = 2; i >= 0; --i) {
            const int k = PMX_BW_S1 + i;
            BW(mask(u, 256, A(k), 256, k));
            if (i > 0) BW(grads2(k, 128, A(k - 1), A(k - 1) + 128, 256));
            else BW(grads2(k, 128, cat + PMX_CAT_FEAT, cat + PMX_CAT_FEAT, PMX_CAT_C));
            BW(dgrad(k, 128, u, u + 128, 256));
        }
        BW(bwd_feat_sum_launch(bw.fg, u, u + 128, 256, n == 1, npix, st));
    }
    BW(mask(bw.fg, 128, cat + PMX_CAT_FEAT, PMX_CAT_C, PMX_BW_C44));
    BW(grads(bw.slot_layer[PMX_BW_C44][0], G(PMX_BW_C44), 128, A(PMX_BW_C43), 256));
    BW(dgrad(PMX_BW_C44, 0, u, nullptr, 256));
    BW(mask(u, 256, A(PMX_BW_C43), 256, PMX_BW_C43));
    BW(grads(bw.slot_layer[PMX_BW_C43][0], G(PMX_BW_C43), 256, A(PMX_BW_X42), 512));
    BW(dgrad(PMX_BW_C43, 0, bw.trunk, nullptr, 512));
    // the concat buffer as the forward left it: the current maps are the last stage's again
    if (n > 1) BW(bwd_copy_cols_launch(A(PMX_BW_M(n, 7)), 64, cat + PMX_CAT_PAF, PMX_CAT_C, npix, 64, st));
#undef BW
    bw.done = true; bw.stepped = false;
    return PMX_OK;
}

extern "C" int pmx_get_layer_grad(pmx_ctx* c, const char* name, float* dw, float* db)
{
    int rc, k, b;
    if ((rc = bw_check(c, "pmx_get_layer_grad", false))) return rc;
    PMX_CHECK(dw || db, PMX_ERR_INVALID, "pmx_get_layer_grad: both outputs are NULL");
    if ((rc = bw_find(c, "pmx_get_layer_grad", name, false, &k, &b)) || (rc = bw_check(c, "pmx_get_layer_grad", true))) return rc;
    PMX_DEV(c);
    const int idx = c->bw.slot_layer[k][b];
    const LayerDesc& d = c->table[idx];
    const size_t nw = (size_t)d.cout * d.cin * d.ks * d.ks;
    const float* src = c->bw.grad + c->bw.grad_off[idx];
    PMX_HIP(hipStreamSynchronize(c->stream));
    if (dw) PMX_HIP(hipMemcpy(dw, src, nw * sizeof(float), hipMemcpyDeviceToHost));
    if (db) PMX_HIP(hipMemcpy(db, src + nw, (size_t)d.cout * sizeof(float), hipMemcpyDeviceToHost));
    return PMX_OK;
}

extern "C" int pmx_get_trunk_grad(pmx_ctx* c, float* g_nchw)
{
    int rc;
    if ((rc = bw_check(c, "pmx_get_trunk_grad", false))) return rc;
    PMX_CHECK(g_nchw, PMX_ERR_INVALID, "pmx_get_trunk_grad: null output");
    if ((rc = bw_check(c, "pmx_get_trunk_grad", true))) return rc;
    PMX_DEV(c);
    return fetch_nchw(c, c->bw.trunk, 512, 512, g_nchw);
}

extern "C" int pmx_get_retained(pmx_ctx* c, const char* name, int which, float* out)
{
    int rc, k, b;
    if ((rc = bw_check(c, "pmx_get_retained", false))) return rc;
    PMX_CHECK(out && (which == 0 || which == 1), PMX_ERR_INVALID, "pmx_get_retained: null output or which = %d outside {0, 1}", which);
    if ((rc = bw_find(c, "pmx_get_retained", name, which == 0, &k, &b))) return rc;
    if (which == 1 && (rc = bw_check(c, "pmx_get_retained", true))) return rc;
    PMX_DEV(c);
    const BwState& bw = c->bw;
    const int C = c->table[bw.slot_layer[k][b]].cout;
    if (which == 1) return fetch_nchw(c, bw.g + bw.slot[k].g_off + (size_t)b * (stage_out(k) ? 64 : C), bw.slot[k].ldg, C, out);
    if (k == PMX_BW_C44) return fetch_nchw(c, c->cat + PMX_CAT_FEAT, PMX_CAT_C, C, out);
    return fetch_nchw(c, bw.act + bw.slot[k].a_off + (size_t)b * (stage_out(k) ? PMX_CAT_HEAT - PMX_CAT_PAF : C), bw.slot[k].lda, C, out);
}
