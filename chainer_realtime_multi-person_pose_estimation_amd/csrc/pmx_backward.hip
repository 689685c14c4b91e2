// pmx_backward.hip -- the head and the trunk backward of the C ABI: pmx_backward_enable / pmx_backward_head / pmx_backward_trunk /
// pmx_get_layer_grad / pmx_get_trunk_grad / pmx_get_retained and the test entries pmx_conv1_wgrad / pmx_pool_backward_test.  Semantics and the orders of every sum: include/pose_mi355x.h; the stores' layout: pmx_ctx.h (BwState); the forward's
// side of retention: pmx_api.hip (pmx_forward_from_in16).  This file holds no kernel: the data gradients are plans of the forward's
// dispatcher on transposed packs (pmx_run_conv), everything else is a launch of conv_bwd.hip.
#include "pmx_ctx.h"

#include <stdio.h>
#include <string.h>
#include <algorithm>

// conv1_1 .. conv4_2 (CocoPoseNet.py:136-149): F.max_pooling_2d follows conv1_2, conv2_2 and conv3_4
const TrunkDesc pmx_trunk_desc[PMX_TRUNK_LAYERS] = {
    {"conv1_1", 3, 64, 0, 0}, {"conv1_2", 64, 64, 0, 1}, {"conv2_1", 64, 128, 1, 0}, {"conv2_2", 128, 128, 1, 1}, {"conv3_1", 128, 256, 2, 0},
    {"conv3_2", 256, 256, 2, 0}, {"conv3_3", 256, 256, 2, 0}, {"conv3_4", 256, 256, 2, 1}, {"conv4_1", 256, 512, 3, 0}, {"conv4_2", 512, 512, 3, 0}};

namespace {

constexpr int N_LG = PMX_N_PAF + PMX_N_HEAT;      // floats per pixel of a stage's loss gradient (pmx_loss.hip)

bool stage_out(int k) { return k == PMX_BW_S1 + 4 || (k >= PMX_BW_M2 && k < PMX_BW_X42 && (k - PMX_BW_M2) % 7 == 6); }
int slot_stage(int k) { return k < PMX_BW_S1 ? 0 : k < PMX_BW_M2 ? 1 : k < PMX_BW_X42 ? 2 + (k - PMX_BW_M2) / 7 : 0; }

// names, leading dimensions and offsets of the slots, the gradient store's offsets, then the allocations; mode 2: the trunk's as well
int bw_layout(pmx_ctx* c, int mode)
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
    // the trunk (mode 2): the store of the pre-pool outputs and the pooled maps, the per-layer g slots (option "trunk_keep_g") and, after
    // every head layer's, the gradient segments.  Level l holds cap0 / 4^l pixels; every offset is a multiple of 64 floats.
    const size_t cap0 = bw.cap_px * 64, pair = mode == 2 ? cap0 * 64 : 0;
    size_t ta = 0, tg = 0;
    if (mode == 2) {
        int pools = 0;
        for (int t = 0; t < PMX_TRUNK_LAYERS; ++t) {
            const TrunkDesc& d = pmx_trunk_desc[t];
            auto it = c->index.find(d.name);
            PMX_CHECK(it != c->index.end() && c->table[it->second].cin == d.cin && c->table[it->second].cout == d.cout && c->table[it->second].ks == 3,
                      PMX_ERR_STATE, "backward: no trunk layer '%s' of %d -> %d channels", d.name, d.cin, d.cout);
            bw.t_layer[t] = it->second;
            const size_t px = cap0 >> (2 * d.level);
            if (t < PMX_TRUNK_LAYERS - 1) { bw.t_a_off[t] = ta; ta += px * d.cout; }
            if (d.pool) { bw.t_p_off[pools++] = ta; ta += px / 4 * d.cout; }
            bw.t_g_off[t] = tg; tg += px * d.cout;
            bw.grad_off[it->second] = off;
            off += ((size_t)d.cout * d.cin * 9 + d.cout + 63) / 64 * 64;
        }
        if (!c->opt_trunk_keep_g) tg = 0;
    }
    // a refused allocation is a capacity error of this context's size, not a runtime failure
    DevBuf<float>* const bufs[] = {&bw.act, &bw.g, &bw.grad, &bw.u, &bw.dcat, &bw.fg, &bw.trunk, &bw.t_act, &bw.t_u, &bw.t_g, &bw.t_gk};
    const size_t counts[] = {a, g, off, bw.cap_px * 1024, bw.cap_px * 2 * PMX_CAT_C, bw.cap_px * 128, bw.cap_px * 512, ta, pair, tg ? 0 : pair, tg};
    bool ok = true;
    for (int i = 0; i < (mode == 2 ? 11 : 7) && ok; ++i) ok = bufs[i]->alloc(counts[i]) == PMX_OK;
    ok = ok && bw.part.alloc((size_t)PMX_DB_SLOTS * 1024) == PMX_OK && bw.cat_of_ref.alloc(185) == PMX_OK;
    if (!ok) {
        (void)hipGetLastError();
        if (mode == 2)
            pmx_set_error("pmx_backward_enable: the device has no room for the stores of %d x %d x %d (%.2f GB of activations, %.2f GB of gradients; "
                          "the trunk: %.2f GB of activations, %.2f GB of gradients)", c->max_batch, c->max_h, c->max_w, a * 4e-9, g * 4e-9, ta * 4e-9,
                          (pair + (tg ? tg : pair)) * 4e-9);
        else
            pmx_set_error("pmx_backward_enable: the device has no room for the stores of %d x %d x %d (%.2f GB of activations, %.2f GB of gradients)",
                          c->max_batch, c->max_h, c->max_w, a * 4e-9, g * 4e-9);
        return PMX_ERR_CAPACITY;
    }
    if (mode == 2) {
        PMX_HIP(hipMemsetAsync(bw.t_u, 0xFF, pair * sizeof(float), c->stream));
        if (tg) PMX_HIP(hipMemsetAsync(bw.t_gk, 0xFF, tg * sizeof(float), c->stream));
        else PMX_HIP(hipMemsetAsync(bw.t_g, 0xFF, pair * sizeof(float), c->stream));
    }
    // poison: an element the backward fails to write is caught by the tests
    PMX_HIP(hipMemsetAsync(bw.g, 0xFF, g * sizeof(float), c->stream));
    PMX_HIP(hipMemsetAsync(bw.grad, 0xFF, off * sizeof(float), c->stream));
    PMX_HIP(hipMemsetAsync(bw.trunk, 0xFF, bw.cap_px * 512 * sizeof(float), c->stream));
    int map[185];
    for (int i = 0; i < 185; ++i) map[i] = pmx_pk_packed_of_ref(1, i);
    PMX_HIP(hipMemcpy(bw.cat_of_ref, map, sizeof map, hipMemcpyHostToDevice));
    return PMX_OK;
}

void bw_free(BwState& bw)
{
    bw.act.reset(); bw.g.reset(); bw.grad.reset(); bw.u.reset(); bw.dcat.reset(); bw.fg.reset(); bw.trunk.reset(); bw.ws.reset(); bw.part.reset();
    bw.cat_of_ref.reset();
    bw.t_act.reset(); bw.t_u.reset(); bw.t_g.reset(); bw.t_gk.reset();
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

// NHWC device (C channels from `src`, ld floats per pixel, h x w pixels per image) -> NCHW host
int fetch_nchw_hw(pmx_ctx* c, const float* src, int ld, int C, int h, int w, float* out)
{
    const size_t n = (size_t)c->bw.B * C * h * w;
    DevBuf<float> tmp;
    int rc;
    if ((rc = tmp.alloc(n)) || (rc = launch_nhwc_to_nchw(src, tmp, c->bw.B, C, h, w, ld, 0, c->stream))) return rc;
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(out, tmp, n * sizeof(float), hipMemcpyDeviceToHost));
    return PMX_OK;
}
int fetch_nchw(pmx_ctx* c, const float* src, int ld, int C, float* out) { return fetch_nchw_hw(c, src, ld, C, c->bw.fh, c->bw.fw, out); }

// the position of a trunk layer in pmx_trunk_desc, -1 for any other name
int trunk_find(const char* name)
{
    for (int t = 0; name && t < PMX_TRUNK_LAYERS; ++t)
        if (!strcmp(name, pmx_trunk_desc[t].name)) return t;
    return -1;
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
        bw.on = 0; bw.valid = bw.done = bw.trunk_done = false;
        return PMX_OK;
    }
    const int mode = on == 2 ? 2 : 1;
    PMX_CHECK(!bw.on || bw.on == mode, PMX_ERR_STATE, "pmx_backward_enable: mode %d asked for while mode %d is on; switch retention off first", mode, bw.on);
    if (bw.on) return PMX_OK;
    if (bw.tl.size() != c->layers.size()) bw.tl.resize(c->layers.size());
    if (int rc = bw_layout(c, mode)) { bw_free(bw); return rc; }
    bw.on = mode; bw.valid = bw.done = bw.trunk_done = false;
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
    // option "grad_precision" = 2: dw and dx of the 3x3 / 7x7 layers with f16 operands (conv_wgrad_f16_launch; the dispatcher's f16 form on the
    // transposed pack); the 1x1 layers, every db and every elementwise step keep their fp32 launches
    auto f16_layer = [&](int idx) { return c->opt_grad_precision == 2 && c->table[idx].ks > 1; };
    auto strips_of = [&](int idx, int cg, int cx, int* rows) {      // (the rule of the kernel that will run: the f16 rule gives more strips)
        const LayerDesc& d = c->table[idx];
        return f16_layer(idx) ? conv_wgrad_f16_strips(B, fh, cg, cx, d.ks, c->opt_wgrad_strips, rows)
                              : conv_wgrad_strips(B, fh, cg, cx, d.ks, c->opt_wgrad_strips, rows);
    };
    // before anything is enqueued: the data-gradient packs (with their f16 packs where the f16 form will read them) and the workspace of the
    // widest weight gradient
    size_t ws_need = 0;
    for (int k = 0; k < PMX_BW_X42; ++k) {
        if (slot_stage(k) > n) continue;
        for (int b = 0; b < 2; ++b) {
            const int idx = bw.slot_layer[k][b];
            if ((rc = pmx_bw_transposed_pack(c, idx, f16_layer(idx)))) return rc;
            const LayerDesc& d = c->table[idx];
            const int cg = round_up(d.cout, 32), cx = round_up(d.cin, 32);
            int rows = 0;
            const int strips = strips_of(idx, cg, cx, &rows);
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
        const int strips = strips_of(idx, cg, cx, &rows);
        if (int r = conv_bwd_db_launch(g, ldg, bw.part, db, npix, d.cout, cg, st)) return r;
        return (f16_layer(idx) ? conv_wgrad_f16_launch : conv_wgrad_launch)(g, ldg, x, ldx, bw.ws, dw, B, fh, fw, d.cout, cg, d.cin, cx, d.ks, strips, rows,
                                                                            d.cin == 185 ? bw.cat_of_ref.get() : nullptr, st, PMX_WGRAD_MAX_STRIPS);
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
        const ConvBuf g = o1 ? ConvBuf::two(G(k), goff, bw.slot[k].ldg) : ConvBuf::one(G(k), bw.slot[k].ldg);
        return pmx_run_conv(c, label, &bw.tl[i0], o1 ? &bw.tl[i1] : nullptr, conv_io(g, ConvBuf{{o0, o1}, ldc}, B, fh, fw, 0, 0), f16_layer(i0) ? 2 : -1);
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
    bw.done = true; bw.stepped = false; bw.trunk_done = false;
    return PMX_OK;
}

// The trunk chain (include/pose_mi355x.h): conv4_2 .. conv1_1 from bw.trunk.  Every trunk output has one consumer, so u of a layer is the dx
// of the layer after it: one buffer for u, one for g (or the layer's own g slot with "trunk_keep_g").
extern "C" int pmx_backward_trunk(pmx_ctx* c)
{
    int rc;
    if ((rc = bw_check(c, "pmx_backward_trunk", true))) return rc;
    PMX_CHECK(c->bw.on == 2, PMX_ERR_STATE, "pmx_backward_trunk: the trunk is not retained (pmx_backward_enable(ctx, 2))");
    PMX_DEV(c);
    BwState& bw = c->bw;
    const int B = bw.B, H = bw.t_H, W = bw.t_W;
    hipStream_t st = c->stream;
    // before anything is enqueued: the data-gradient packs (conv1_1 has no dx), the strips and the workspace of the widest weight gradient
    int strips[PMX_TRUNK_LAYERS], rows[PMX_TRUNK_LAYERS];
    size_t ws_need = 0;
    for (int t = 0; t < PMX_TRUNK_LAYERS; ++t) {
        const TrunkDesc& d = pmx_trunk_desc[t];
        if (t == 0) {
            strips[t] = conv1_wgrad_strips(B, H, c->opt_wgrad_strips, &rows[t]);
            ws_need = std::max(ws_need, (size_t)strips[t] * 64 * 32);
            continue;
        }
        if ((rc = pmx_bw_transposed_pack(c, bw.t_layer[t]))) return rc;
        strips[t] = conv_wgrad_trunk_strips(B, H >> d.level, d.cout, d.cin, c->opt_wgrad_strips, &rows[t]);
        ws_need = std::max(ws_need, (size_t)strips[t] * 9 * d.cout * d.cin);
    }
    if ((rc = bw.ws.ensure(ws_need, st))) return rc;
    auto pooled_of = [&](int t) { return bw.t_act + bw.t_p_off[t == 1 ? 0 : t == 3 ? 1 : 2]; };
    const float* u = bw.trunk;
    char label[64];
#define BW(x) do { if ((rc = (x))) return rc; } while (0)
    for (int t = PMX_TRUNK_LAYERS - 1; t >= 0; --t) {
        const TrunkDesc& d = pmx_trunk_desc[t];
        const int idx = bw.t_layer[t], h = H >> d.level, w = W >> d.level;
        const long long npix = (long long)B * h * w;
        const float* a = t == PMX_TRUNK_LAYERS - 1 ? bw.act + bw.slot[PMX_BW_X42].a_off : bw.t_act + bw.t_a_off[t];
        const float* x = t == 0 ? c->in16.get() : pmx_trunk_desc[t - 1].pool ? pooled_of(t - 1) : bw.t_act + bw.t_a_off[t - 1];
        float* g = bw.t_gk.capacity() ? bw.t_gk + bw.t_g_off[t] : bw.t_g.get();
        float* dw = bw.grad + bw.grad_off[idx];
        float* db = dw + (size_t)d.cout * d.cin * 9;
        snprintf(label, sizeof label, "bwd_g:%s|%s", d.name, d.pool ? "pool_bwd_db" : "mask_db");
        BW(pmx_prof_begin(c, label, 4.0 * npix * d.cout * (d.pool ? 3.25 : 4.0)));
        // (a pooled layer's u has the pooled size: it is the dx of the next layer, which read the pooled map)
        if (d.pool) BW(pool_bwd_nhwc_launch(u, d.cout, a, d.cout, g, d.cout, B, h, w, d.cout, st));
        else BW(bwd_mask_nhwc_launch(u, d.cout, a, d.cout, g, d.cout, npix, d.cout, st));
        BW(conv_bwd_db_launch(g, d.cout, bw.part, db, npix, d.cout, d.cout, st));
        BW(pmx_prof_end(c));
        snprintf(label, sizeof label, "bwd_dw:%s|%s", d.name, t == 0 ? "conv1_wgrad" : "conv_wgrad");
        BW(pmx_prof_begin(c, label, 4.0 * npix * (d.cout + (t == 0 ? PMX_IN_C : d.cin))));
        if (t == 0) BW(conv1_wgrad_launch(g, 64, x, bw.ws, dw, B, h, w, strips[t], rows[t], st));
        else BW(conv_wgrad_launch(g, d.cout, x, d.cin, bw.ws, dw, B, h, w, d.cout, d.cout, d.cin, d.cin, 3, strips[t], rows[t], nullptr, st,
                                  2 * PMX_WGRAD_TRUNK_MAX_STRIPS));
        BW(pmx_prof_end(c));
        if (t == 0) break;
        snprintf(label, sizeof label, "bwd_dx:%s", d.name);
        BW(pmx_run_conv(c, label, &bw.tl[idx], nullptr, conv_io(ConvBuf::one(g, d.cout), ConvBuf::one(bw.t_u, d.cin), B, h, w, 0, 0)));
        u = bw.t_u;
    }
#undef BW
    bw.trunk_done = true;
    return PMX_OK;
}

extern "C" int pmx_get_layer_grad(pmx_ctx* c, const char* name, float* dw, float* db)
{
    int rc, k, b;
    if ((rc = bw_check(c, "pmx_get_layer_grad", false))) return rc;
    PMX_CHECK(dw || db, PMX_ERR_INVALID, "pmx_get_layer_grad: both outputs are NULL");
    if (c->bw.on == 2 && trunk_find(name) >= 0) {
        PMX_CHECK(c->bw.done && c->bw.trunk_done, PMX_ERR_STATE, "pmx_get_layer_grad: pmx_backward_trunk has not run for the retained forward");
        PMX_DEV(c);
        const TrunkDesc& d = pmx_trunk_desc[trunk_find(name)];
        const size_t nw = (size_t)d.cout * d.cin * 9;
        const float* src = c->bw.grad + c->bw.grad_off[c->bw.t_layer[trunk_find(name)]];
        PMX_HIP(hipStreamSynchronize(c->stream));
        if (dw) PMX_HIP(hipMemcpy(dw, src, nw * sizeof(float), hipMemcpyDeviceToHost));
        if (db) PMX_HIP(hipMemcpy(db, src + nw, (size_t)d.cout * sizeof(float), hipMemcpyDeviceToHost));
        return PMX_OK;
    }
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
    const int t = c->bw.on == 2 ? trunk_find(name) : -1;
    if (out && c->bw.on == 2 && name && !strcmp(name, "input") && which == 0) {      // the prepared input, 3 real channels of PMX_IN_C
        PMX_DEV(c);
        return fetch_nchw_hw(c, c->in16, PMX_IN_C, 3, c->bw.t_H, c->bw.t_W, out);
    }
    if (out && t >= 0 && !(t == PMX_TRUNK_LAYERS - 1 && which == 0)) {               // (conv4_2's a: the slot of mode 1, below)
        const BwState& bw = c->bw;
        const TrunkDesc& d = pmx_trunk_desc[t];
        const int h = bw.t_H >> d.level, w = bw.t_W >> d.level;
        PMX_CHECK(which == 0 || which == 1 || (which == 2 && d.pool), PMX_ERR_INVALID, "pmx_get_retained: which = %d for trunk layer '%s' (2: the pooled map of "
                  "conv1_2, conv2_2, conv3_4 only)", which, name);
        PMX_DEV(c);
        if (which == 0) return fetch_nchw_hw(c, bw.t_act + bw.t_a_off[t], d.cout, d.cout, h, w, out);
        if (which == 2) return fetch_nchw_hw(c, bw.t_act + bw.t_p_off[t == 1 ? 0 : t == 3 ? 1 : 2], d.cout, d.cout, h / 2, w / 2, out);
        PMX_CHECK(bw.done && bw.trunk_done, PMX_ERR_STATE, "pmx_get_retained: pmx_backward_trunk has not run for the retained forward");
        PMX_CHECK(bw.t_gk.capacity(), PMX_ERR_STATE, "pmx_get_retained: the g of a trunk layer is kept only with option \"trunk_keep_g\" set before "
                  "pmx_backward_enable(ctx, 2)");
        return fetch_nchw_hw(c, bw.t_gk + bw.t_g_off[t], d.cout, d.cout, h, w, out);
    }
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

// The range census of one head layer's kept g (include/pose_mi355x.h): a launch of its own, on request only -- never part of the chain.
extern "C" int pmx_backward_g_census(pmx_ctx* c, const char* name, unsigned long long counts[5])
{
    int rc, k, b;
    if ((rc = bw_check(c, "pmx_backward_g_census", false))) return rc;
    PMX_CHECK(counts, PMX_ERR_INVALID, "pmx_backward_g_census: null output");
    if ((rc = bw_find(c, "pmx_backward_g_census", name, false, &k, &b)) || (rc = bw_check(c, "pmx_backward_g_census", true))) return rc;
    PMX_DEV(c);
    const BwState& bw = c->bw;
    const int C = c->table[bw.slot_layer[k][b]].cout;
    DevBuf<unsigned long long> d;
    if ((rc = d.alloc(5))) return rc;
    PMX_HIP(hipMemsetAsync(d, 0, 5 * sizeof(unsigned long long), c->stream));
    rc = bwd_g_census_launch(bw.g + bw.slot[k].g_off + (size_t)b * (stage_out(k) ? 64 : C), bw.slot[k].ldg, (long long)bw.B * bw.fh * bw.fw, C, d, c->stream);
    PMX_HIP(hipStreamSynchronize(c->stream));               // (nothing in flight may outlive the buffer)
    if (rc) return rc;
    PMX_HIP(hipMemcpy(counts, d, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PMX_OK;
}

// ---- test entries: the trunk backward's own kernels on the caller's arrays (include/pose_mi355x.h) --------------------------------------
extern "C" int pmx_conv1_wgrad(pmx_ctx* c, const float* x_nchw, const float* g_nchw, int B, int H, int W, int strips, float* dw_oihw, int* strips_out,
                               int* rows_out)
{
    PMX_CHECK(c && x_nchw && g_nchw && dw_oihw, PMX_ERR_INVALID, "pmx_conv1_wgrad: null arg");
    PMX_CHECK(B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W >= 2 && (long long)B * H * W < (1ll << 31) / 64, PMX_ERR_INVALID,
              "pmx_conv1_wgrad: bad shape %d x %d x %d", B, H, W);
    PMX_DEV(c);
    const size_t npix = (size_t)B * H * W;
    int rows = 0, rc;
    const int S = conv1_wgrad_strips(B, H, strips, &rows);
    DevBuf<float> d_in, d_x, d_g, d_ws, d_dw;
    if ((rc = d_in.alloc(npix * 64)) || (rc = d_x.alloc(npix * PMX_IN_C)) || (rc = d_g.alloc(npix * 64)) || (rc = d_ws.alloc((size_t)S * 64 * 32)) ||
        (rc = d_dw.alloc(64 * 27))) return rc;
    hipStream_t st = c->stream;
    auto run = [&]() -> int {
        int r;
        PMX_HIP(hipMemcpyAsync(d_in, x_nchw, npix * 3 * sizeof(float), hipMemcpyHostToDevice, st));
        PMX_HIP(hipMemsetAsync(d_x, 0, npix * PMX_IN_C * sizeof(float), st));
        if ((r = launch_nchw_to_nhwc(d_in, d_x, B, 3, H, W, PMX_IN_C, 0, st))) return r;
        PMX_HIP(hipStreamSynchronize(st));                  // (d_in is reused for g; the host arrays are pageable)
        PMX_HIP(hipMemcpyAsync(d_in, g_nchw, npix * 64 * sizeof(float), hipMemcpyHostToDevice, st));
        if ((r = launch_nchw_to_nhwc(d_in, d_g, B, 64, H, W, 64, 0, st))) return r;
        PMX_HIP(hipMemsetAsync(d_dw, 0xFF, 64 * 27 * sizeof(float), st));
        PMX_HIP(hipMemsetAsync(d_ws, 0xFF, (size_t)S * 64 * 32 * sizeof(float), st));
        if ((r = conv1_wgrad_launch(d_g, 64, d_x, d_ws, d_dw, B, H, W, S, rows, st))) return r;
        PMX_HIP(hipStreamSynchronize(st));
        PMX_HIP(hipMemcpy(dw_oihw, d_dw, 64 * 27 * sizeof(float), hipMemcpyDeviceToHost));
        return PMX_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);                 // nothing in flight may outlive the buffers
    if (strips_out) *strips_out = S;
    if (rows_out) *rows_out = rows;
    return rc;
}

extern "C" int pmx_pool_backward_test(pmx_ctx* c, const float* a_nchw, const float* u_nchw, int B, int C, int H, int W, float* pooled_out, float* g_out)
{
    PMX_CHECK(c && a_nchw && u_nchw && pooled_out && g_out, PMX_ERR_INVALID, "pmx_pool_backward_test: null arg");
    PMX_CHECK(B >= 1 && C >= 1 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0 && (long long)B * C * H * W < (1ll << 31), PMX_ERR_INVALID,
              "pmx_pool_backward_test: bad shape %d x %d x %d x %d (H, W even)", B, C, H, W);
    PMX_DEV(c);
    const size_t n = (size_t)B * C * H * W;
    DevBuf<float> d_in, d_a, d_u, d_p, d_g, d_out;
    int rc;
    if ((rc = d_in.alloc(n)) || (rc = d_a.alloc(n)) || (rc = d_u.alloc(n / 4)) || (rc = d_p.alloc(n / 4)) || (rc = d_g.alloc(n)) || (rc = d_out.alloc(n))) return rc;
    hipStream_t st = c->stream;
    auto run = [&]() -> int {
        int r;
        PMX_HIP(hipMemcpyAsync(d_in, a_nchw, n * sizeof(float), hipMemcpyHostToDevice, st));
        if ((r = launch_nchw_to_nhwc(d_in, d_a, B, C, H, W, C, 0, st))) return r;
        PMX_HIP(hipStreamSynchronize(st));
        PMX_HIP(hipMemcpyAsync(d_in, u_nchw, n / 4 * sizeof(float), hipMemcpyHostToDevice, st));
        if ((r = launch_nchw_to_nhwc(d_in, d_u, B, C, H / 2, W / 2, C, 0, st))) return r;
        PMX_HIP(hipMemsetAsync(d_p, 0xFF, n / 4 * sizeof(float), st));
        PMX_HIP(hipMemsetAsync(d_g, 0xFF, n * sizeof(float), st));
        if ((r = maxpool_nhwc_launch(d_a, C, d_p, C, B, H, W, C, st)) || (r = pool_bwd_nhwc_launch(d_u, C, d_a, C, d_g, C, B, H, W, C, st))) return r;
        if ((r = launch_nhwc_to_nchw(d_p, d_out, B, C, H / 2, W / 2, C, 0, st))) return r;
        PMX_HIP(hipStreamSynchronize(st));
        PMX_HIP(hipMemcpy(pooled_out, d_out, n / 4 * sizeof(float), hipMemcpyDeviceToHost));
        if ((r = launch_nhwc_to_nchw(d_g, d_out, B, C, H, W, C, 0, st))) return r;
        PMX_HIP(hipStreamSynchronize(st));
        PMX_HIP(hipMemcpy(g_out, d_out, n * sizeof(float), hipMemcpyDeviceToHost));
        return PMX_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
}
