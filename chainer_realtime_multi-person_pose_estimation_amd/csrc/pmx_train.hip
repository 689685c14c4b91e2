// pmx_train.hip -- the training steps of the C ABI: pmx_train_enable / pmx_train_set_adam / pmx_train_set_grad_scale /
// pmx_train_step_head / pmx_train_step / pmx_get_layer / pmx_train_get_state / pmx_train_set_state / pmx_get_pack /
// pmx_get_transposed_f16_pack / pmx_adam_apply.  Semantics:
// include/pose_mi355x.h; the stores' layout: pmx_ctx.h (TrainState, BwState::grad); every pack: pack_index.h, built by pmx_packs.hip.
//
// THE ADAM CONTRACT is this project's own restatement of Chainer's AdamRule (eta = 1, weight_decay_rate = 0) as a sequence of float32
// operations, each rounded to nearest -- see adam_one below.  A CUDA build of Chainer may contract a multiply and an add into one FMA, so
// bit equality with Chainer is NOT claimed; bit equality with tests/adam_twin.py is.  This unit is compiled with -ffp-contract=off (nothing is
// fused) and -fhip-fp32-correctly-rounded-divide-sqrt (the float32 `/` and sqrt below expand to the correctly rounded sequences whatever the
// compiler's default is; HIP's __fsqrt_rn is the 1-ulp hardware square root unless OCML's rounded operations are compiled in, so it is not used).
#include "pmx_ctx.h"

#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_ITERS = 4;                                             // 16-byte vectors per lane
constexpr unsigned ADAM_BLOCK_FLOATS = ADAM_THREADS * ADAM_ITERS * 4;     // floats of a segment one block covers

__device__ __forceinline__ float rn_div(float a, float b) { return __fdiv_rn(a, b); }          // a / b, correctly rounded (flag above)
__device__ __forceinline__ float rn_sqrt(float a) { return __builtin_sqrtf(a); }               // correctly rounded (flag above)

// one parameter: every line one float32 operation
__device__ __forceinline__ float adam_one(float grad, float w, float& m, float& v, float scale, float alpha_t, float omb1, float omb2, float eps)
{
    const float g = grad * scale;
    const float d = g - m;
    const float dm = omb1 * d;
    m = m + dm;
    const float q = g * g;
    const float e = q - v;
    const float dv = omb2 * e;
    v = v + dv;
    const float r = rn_sqrt(v);
    const float s = r + eps;
    const float am = alpha_t * m;
    const float u = rn_div(am, s);
    return w - u;
}

// The whole store in one launch.  Block b serves the segment whose [blk0, next blk0) holds b (at most 92 segments: seven steps of a search), floats
// (b - blk0) * ADAM_BLOCK_FLOATS ... of it.  Every segment starts at a multiple of 64 floats and is padded to one, so each lane moves whole
// 16-byte vectors; the lanes of the last vector past n keep the bits they loaded (a pad float is never used as a parameter, never changed).
__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                                                            const float* __restrict__ grad, const AdamSeg* __restrict__ segs, int nseg,
                                                            float omb1, float omb2, float eps)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].blk0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const AdamSeg s = segs[lo];
    const unsigned base = (blockIdx.x - s.blk0) * ADAM_BLOCK_FLOATS;
#pragma unroll
    for (int it = 0; it < ADAM_ITERS; ++it) {
        const unsigned i = base + (unsigned)(it * ADAM_THREADS + threadIdx.x) * 4u;
        if (i >= s.n) return;
        const size_t at = (size_t)s.off + i;
        const float4 g4 = *reinterpret_cast<const float4*>(grad + at);
        float4 w4 = *reinterpret_cast<const float4*>(w + at);
        float4 m4 = *reinterpret_cast<const float4*>(m + at);
        float4 v4 = *reinterpret_cast<const float4*>(v + at);
        const float gg[4] = {g4.x, g4.y, g4.z, g4.w};
        float ww[4] = {w4.x, w4.y, w4.z, w4.w}, mm[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mk = mm[k], vk = vv[k];
            const float wk = adam_one(gg[k], ww[k], mk, vk, s.scale, s.alpha_t, omb1, omb2, eps);
            if (i + k < s.n) { ww[k] = wk; mm[k] = mk; vv[k] = vk; }
        }
        *reinterpret_cast<float4*>(w + at) = make_float4(ww[0], ww[1], ww[2], ww[3]);
        *reinterpret_cast<float4*>(m + at) = make_float4(mm[0], mm[1], mm[2], mm[3]);
        *reinterpret_cast<float4*>(v + at) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    }
}

#define TR_LAUNCHED(what) do { const hipError_t _e = hipGetLastError(); \
    if (_e != hipSuccess) { pmx_set_error("%s: launch failed: %s", what, hipGetErrorString(_e)); return PMX_ERR_HIP; } } while (0)

// the stage of a head layer (0: conv4_3_CPM / conv4_4_CPM), -1 for a layer the head backward does not cover
int head_stage(const pmx_ctx* c, int idx)
{
    if ((size_t)idx >= c->bw.layer_slot.size() || c->bw.layer_slot[idx] < 0) return -1;
    const int k = c->bw.layer_slot[idx] / 2;
    return k < PMX_BW_S1 ? 0 : k < PMX_BW_M2 ? 1 : 2 + (k - PMX_BW_M2) / 7;
}

// the position 0 .. 9 of a trunk layer (conv1_1 .. conv4_2) while the trunk is retained (mode 2: it has a gradient segment), else -1
int trunk_pos(const pmx_ctx* c, int idx)
{
    if (c->bw.on != 2) return -1;
    for (int t = 0; t < PMX_TRUNK_LAYERS; ++t)
        if (c->bw.t_layer[t] == idx) return t;
    return -1;
}

// a layer with a segment in the stores: the 82 head layers, in mode 2 the ten trunk layers as well
bool has_segment(const pmx_ctx* c, int idx) { return head_stage(c, idx) >= 0 || trunk_pos(c, idx) >= 0; }

// The tables of one step in the pinned block (and, at the same offsets, in its device copy): the Adam segments, then the jobs of the
// packer launches kind by kind (pmx_packs.hip), each kind with room for what N layers can give it (PMX_PACK_JOBS_PER_LAYER).
size_t jobs_at(size_t N, int kind)
{
    size_t jobs = 0;
    for (int k = 0; k < kind; ++k) jobs += PMX_PACK_JOBS_PER_LAYER[k] ? PMX_PACK_JOBS_PER_LAYER[k] * N : 1;
    return N * sizeof(AdamSeg) + jobs * sizeof(PackJob);
}
size_t table_bytes(size_t N) { return jobs_at(N, PMX_PACK_KINDS); }

// a job owns the blocks [blk0, next blk0) of its launch, 256 floats of its pack each
struct JobList { PackJob* job; int n = 0; unsigned blocks = 0; };
void add_job(JobList& l, PackJob j)
{
    j.blk0 = l.blocks;
    l.job[l.n++] = j;
    l.blocks += (j.total + 255) / 256;
}

// a pack derived from a direct pack, rewritten in the buffer of `held` elements that holds it
int derived_job(JobList& l, const PackJob& j, size_t held, const char* what)
{
    PMX_CHECK(held == j.total, PMX_ERR_STATE, "training step: %s pack of %zu elements where %u are expected", what, held, j.total);
    add_job(l, j);
    return PMX_OK;
}

int wino_job(JobList& l, const PackedLayer& L)
{
    PMX_CHECK(L.cin_pad % 32 == 0 && L.cout_pad % 32 == 0, PMX_ERR_STATE, "training step: a Winograd pack of a layer with %d x %d padded channels",
              L.cout_pad, L.cin_pad);
    return derived_job(l, pmx_pack_job_wino(L, L.d_ww), L.d_ww.capacity(), "a Winograd");
}

// the jobs of every pack of layer `idx` that exists, from the master weights at `w`; nothing is enqueued and no flag is set
int repack_jobs(pmx_ctx* c, int idx, const float* w, JobList* jl)
{
    const PackedLayer& L = c->layers[idx];
    const int kind = pmx_pack_kind(c, L.cin);
    const PackJob j = pmx_pack_job_direct(w, L, kind);
    PMX_CHECK(L.d_w.capacity() == j.total && L.d_b.capacity() == (size_t)L.cout_pad, PMX_ERR_STATE, "training step: layer '%s': a pack of %zu floats where %u are expected",
              c->table[idx].name.c_str(), L.d_w.capacity(), j.total);
    add_job(jl[PMX_PACK_DIRECT], j);
    int rc;
    if (L.d_w16 && (rc = derived_job(jl[PMX_PACK_F16], pmx_pack_job_f16(L, L.d_w16), L.d_w16.capacity(), "an f16"))) return rc;
    if (L.d_w3 && (rc = derived_job(jl[PMX_PACK_BF16X3], pmx_pack_job_bf16x3(L, L.d_w3), L.d_w3.capacity(), "a bf16x3"))) return rc;
    if (L.d_ww && trunk_pos(c, idx) == 0) {      // conv1_1's Winograd slot holds its fused-kernel pack
        PMX_CHECK(L.d_ww.capacity() == (size_t)PMX_PK_CONV1_FLOATS && L.nch == 1 && L.cout_pad == 64, PMX_ERR_STATE,
                  "training step: conv1_1's fused-kernel pack has %zu floats where %d are expected", L.d_ww.capacity(), PMX_PK_CONV1_FLOATS);
        add_job(jl[PMX_PACK_CONV1], pmx_pack_job_conv1(L, L.d_ww));
    } else if (L.d_ww && (rc = wino_job(jl[PMX_PACK_WINO], L))) return rc;
    if ((size_t)idx >= c->bw.tl.size() || !c->bw.tl[idx].set) return PMX_OK;
    const PackedLayer& P = c->bw.tl[idx];
    const PackJob jt = pmx_pack_job_transposed(w, L.cout, L.cin, L.ks, kind, P);
    PMX_CHECK(P.d_w.capacity() == jt.total && P.cout == pmx_pk_t_cout(kind, L.cin) && P.cin_pad == pmx_pk_t_cin_pad(L.cout), PMX_ERR_STATE,
              "training step: layer '%s': a transposed pack of another shape", c->table[idx].name.c_str());
    add_job(jl[PMX_PACK_TRANSPOSED], jt);
    // (the f16 pack of the transposed layer exists once a head backward ran under "grad_precision" 2: the next one reads the new weights)
    if (P.d_w16 && (rc = derived_job(jl[PMX_PACK_F16], pmx_pack_job_f16(P, P.d_w16), P.d_w16.capacity(), "a transposed f16"))) return rc;
    if (P.d_ww && (rc = wino_job(jl[PMX_PACK_WINO], P))) return rc;
    return PMX_OK;
}

// the packs a step rewrites behind the host's back, and the lazy host builders that must wait for it: every layer with a segment
void mark_busy(pmx_ctx* c, bool on)
{
    for (size_t i = 0; i < c->layers.size(); ++i) {
        if (!has_segment(c, (int)i)) continue;
        c->layers[i].busy = on; c->layers[i].busy_stream = c->stream;
        if (i < c->bw.tl.size()) { c->bw.tl[i].busy = on; c->bw.tl[i].busy_stream = c->stream; }
    }
}

int tr_check(pmx_ctx* c, const char* who, bool need_on)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "%s: null ctx", who);
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "%s: training exists for posenet contexts only", who);
    PMX_CHECK(c->opt_precision == 0, PMX_ERR_STATE, "%s: option \"precision\" is %d; training is fp32 only", who, c->opt_precision);
    PMX_CHECK(!need_on || c->tr.on, PMX_ERR_STATE, "%s: training is off (pmx_train_enable)", who);
    return PMX_OK;
}

// a layer with Adam state: one of the 82 head layers, in mode 2 one of the ten trunk layers as well
int state_layer(pmx_ctx* c, const char* who, const char* name, int* idx)
{
    PMX_CHECK(name, PMX_ERR_INVALID, "%s: null layer name", who);
    auto it = c->index.find(name);
    PMX_CHECK(it != c->index.end() && has_segment(c, it->second), PMX_ERR_INVALID, "%s: '%s' is not one of the 82 layers after conv4_2%s", who, name,
              c->bw.on == 2 ? " or the ten trunk layers" : " (the trunk layers have state with pmx_backward_enable(ctx, 2) only)");
    *idx = it->second;
    return PMX_OK;
}

float alpha_t_of(const TrainState& tr, int t)
{
    return (float)(tr.alpha * sqrt(1.0 - pow(tr.beta2, (double)t)) / (1.0 - pow(tr.beta1, (double)t)));
}

int launch_adam(float* w, float* m, float* v, const float* grad, const AdamSeg* d_segs, int nseg, unsigned blocks, float omb1, float omb2, float eps,
                hipStream_t st)
{
    adam_kernel<<<blocks, ADAM_THREADS, 0, st>>>(w, m, v, grad, d_segs, nseg, omb1, omb2, eps);
    TR_LAUNCHED("adam");
    return PMX_OK;
}

}  // namespace

void pmx_train_free(pmx_ctx* c)
{
    TrainState& tr = c->tr;
    if (!tr.on) return;
    tr.w.reset(); tr.m.reset(); tr.v.reset(); tr.seg.reset();
    mark_busy(c, false);
    tr.on = 0;
}

float* pmx_train_master(const pmx_ctx* c, int layer)
{
    return c->tr.on && has_segment(c, layer) ? c->tr.w + c->bw.grad_off[layer] : nullptr;      // (a trunk layer in mode 1: no segment, no step ever touches it)
}

extern "C" int pmx_train_enable(pmx_ctx* c, int on)
{
    int rc;
    PMX_CHECK(c, PMX_ERR_INVALID, "pmx_train_enable: null ctx");
    PMX_DEV(c);
    TrainState& tr = c->tr;
    if (!on) {
        if (tr.on) { PMX_HIP(hipStreamSynchronize(c->stream)); pmx_train_free(c); }
        return PMX_OK;
    }
    if ((rc = tr_check(c, "pmx_train_enable", false))) return rc;
    if (tr.on) return PMX_OK;
    PMX_CHECK(c->bw.on, PMX_ERR_STATE, "pmx_train_enable: the head backward is off (pmx_backward_enable)");
    if ((rc = pmx_check_weights(c))) return rc;
    const size_t total = c->bw.grad.capacity();
    hipStream_t st = c->stream;
    char *host, *dev;      // (the steps' table is reserved here: a step allocates nothing)
    const bool ok = tr.w.alloc(total) == PMX_OK && tr.m.alloc(total) == PMX_OK && tr.v.alloc(total) == PMX_OK &&
                    tr.seg.begin(table_bytes(c->table.size()), st, &host, &dev) == PMX_OK;
    if (!ok) {
        (void)hipGetLastError();
        tr.w.reset(); tr.m.reset(); tr.v.reset(); tr.seg.reset();
        pmx_set_error("pmx_train_enable: the device has no room for the master weights and the two moments (3 x %.2f GB)", total * 4e-9);
        return PMX_ERR_CAPACITY;
    }
    PMX_HIP(hipMemsetAsync(tr.w, 0, total * sizeof(float), st));
    PMX_HIP(hipMemsetAsync(tr.m, 0, total * sizeof(float), st));
    PMX_HIP(hipMemsetAsync(tr.v, 0, total * sizeof(float), st));
    for (size_t i = 0; i < c->layers.size(); ++i)
        if (has_segment(c, (int)i) && (rc = pmx_unpack_launch(c->layers[i], pmx_pack_kind(c, c->layers[i].cin), tr.w + c->bw.grad_off[i], st))) {
            (void)hipStreamSynchronize(st);
            tr.w.reset(); tr.m.reset(); tr.v.reset(); tr.seg.reset();
            return rc;
        }
    tr.t.assign(c->table.size(), 0);
    tr.scale.assign(c->table.size(), 1.0f);
    tr.alpha = 1e-4; tr.beta1 = 0.9; tr.beta2 = 0.999; tr.eps = 1e-8;
    tr.on = 1;
    mark_busy(c, true);
    return PMX_OK;
}

extern "C" int pmx_train_set_adam(pmx_ctx* c, double alpha, double beta1, double beta2, double eps)
{
    int rc;
    if ((rc = tr_check(c, "pmx_train_set_adam", true))) return rc;
    PMX_CHECK(alpha > 0 && beta1 >= 0 && beta1 < 1 && beta2 >= 0 && beta2 < 1 && eps > 0 && isfinite(alpha) && isfinite(eps), PMX_ERR_INVALID,
              "pmx_train_set_adam: alpha %g, beta1 %g, beta2 %g, eps %g (alpha, eps > 0; 0 <= beta < 1)", alpha, beta1, beta2, eps);
    c->tr.alpha = alpha; c->tr.beta1 = beta1; c->tr.beta2 = beta2; c->tr.eps = eps;
    return PMX_OK;
}

extern "C" int pmx_train_set_grad_scale(pmx_ctx* c, const char* name, double scale)
{
    int rc, idx;
    if ((rc = tr_check(c, "pmx_train_set_grad_scale", true)) || (rc = state_layer(c, "pmx_train_set_grad_scale", name, &idx))) return rc;
    PMX_CHECK(isfinite(scale), PMX_ERR_INVALID, "pmx_train_set_grad_scale: scale %g", scale);
    c->tr.scale[idx] = (float)scale;
    return PMX_OK;
}

// Both steps: `full` adds the ten trunk layers (mode 2, after pmx_backward_trunk).  Everything that can refuse does so before a launch.
static int train_step(pmx_ctx* c, const char* who, bool full)
{
    int rc;
    if ((rc = tr_check(c, who, true))) return rc;
    BwState& bw = c->bw;
    TrainState& tr = c->tr;
    PMX_CHECK(!full || bw.on == 2, PMX_ERR_STATE, "%s: the trunk is not retained (pmx_backward_enable(ctx, 2) before pmx_train_enable)", who);
    PMX_CHECK(bw.on && bw.valid && bw.done, PMX_ERR_STATE, "%s: pmx_backward_head has not run for a retained forward", who);
    PMX_CHECK(!full || bw.trunk_done, PMX_ERR_STATE, "%s: pmx_backward_trunk has not run for the retained forward", who);
    PMX_CHECK(!bw.stepped, PMX_ERR_STATE, "%s: a step has consumed these gradients (run a new retained forward and the backward)", who);
    PMX_DEV(c);
    hipStream_t st = c->stream;
    const size_t N = c->table.size();
    char *host, *dev;      // (reserved by pmx_train_enable: this waits for the last step's copy and allocates nothing)
    if ((rc = tr.seg.begin(table_bytes(N), st, &host, &dev))) return rc;
    AdamSeg* seg = reinterpret_cast<AdamSeg*>(host);
    JobList jl[PMX_PACK_KINDS];
    for (int k = 0; k < PMX_PACK_KINDS; ++k) jl[k].job = reinterpret_cast<PackJob*>(host + jobs_at(N, k));
    auto updated = [&](int i) {      // (a stage that "stop_stage" cut off received no gradient; the trunk always does)
        const int stage = head_stage(c, i);
        return stage >= 0 ? stage <= bw.stages : full && trunk_pos(c, i) >= 0;
    };
    for (size_t i = 0; i < N; ++i)
        if (updated((int)i) && (rc = repack_jobs(c, (int)i, tr.w + bw.grad_off[i], jl))) return rc;
    int nseg = 0;
    unsigned blocks = 0;
    double bytes = 0;
    for (size_t i = 0; i < N; ++i) {
        if (!updated((int)i)) continue;
        const LayerDesc& d = c->table[i];
        const unsigned n = (unsigned)((size_t)d.cout * d.cin * d.ks * d.ks + d.cout);
        tr.t[i] += 1;
        seg[nseg++] = AdamSeg{(unsigned long long)bw.grad_off[i], n, blocks, tr.scale[i], alpha_t_of(tr, tr.t[i])};
        blocks += (n + ADAM_BLOCK_FLOATS - 1) / ADAM_BLOCK_FLOATS;
        bytes += 28.0 * n;
    }
    bw.stepped = true;
    mark_busy(c, true);
    if ((rc = tr.seg.commit(table_bytes(N), st))) return rc;
    if ((rc = pmx_prof_begin(c, "train_step|adam", bytes))) return rc;
    rc = launch_adam(tr.w, tr.m, tr.v, bw.grad, reinterpret_cast<const AdamSeg*>(dev), nseg, blocks, (float)(1.0 - tr.beta1),
                     (float)(1.0 - tr.beta2), (float)tr.eps, st);
    if (int r = pmx_prof_end(c)) return r;
    if (rc) return rc;
    // the packers, in the order of their inputs: the direct and transposed packs read the master weights, the f16, bf16x3, Winograd and
    // conv1_1 packs the direct packs just written -- and the f16 and Winograd packs of a transposed layer the transposed pack just written,
    // so the transposed packs go before the f16 ones
    static const int order[PMX_PACK_KINDS] = {PMX_PACK_DIRECT, PMX_PACK_TRANSPOSED, PMX_PACK_F16, PMX_PACK_BF16X3, PMX_PACK_WINO, PMX_PACK_CONV1};
    if ((rc = pmx_prof_begin(c, "train_step|pack", 0))) return rc;
    for (int i = 0; i < PMX_PACK_KINDS && !rc; ++i)
        if (const int k = order[i]; jl[k].n) rc = pmx_pack_launch_table(k, reinterpret_cast<const PackJob*>(dev + jobs_at(N, k)), jl[k].n, jl[k].blocks, st);
    if (int r = pmx_prof_end(c)) return r;
    return rc;
}

extern "C" int pmx_train_step_head(pmx_ctx* c) { return train_step(c, "pmx_train_step_head", false); }
extern "C" int pmx_train_step(pmx_ctx* c) { return train_step(c, "pmx_train_step", true); }

extern "C" int pmx_get_layer(pmx_ctx* c, const char* name, float* w_oihw, float* bias)
{
    PMX_CHECK(c && name, PMX_ERR_INVALID, "pmx_get_layer: null arg");
    PMX_CHECK(w_oihw || bias, PMX_ERR_INVALID, "pmx_get_layer: both outputs are NULL");
    auto it = c->index.find(name);
    PMX_CHECK(it != c->index.end(), PMX_ERR_INVALID, "pmx_get_layer: unknown layer '%s'", name);
    const int idx = it->second;
    const PackedLayer& L = c->layers[idx];
    PMX_CHECK(L.set, PMX_ERR_WEIGHTS, "pmx_get_layer: layer '%s' has no weights", name);
    PMX_DEV(c);
    const size_t nw = (size_t)L.cout * L.cin * L.ks * L.ks;
    DevBuf<float> tmp;
    const float* src = pmx_train_master(c, idx);
    if (!src) {
        int rc;
        if ((rc = tmp.alloc(nw + L.cout)) || (rc = pmx_unpack_launch(L, pmx_pack_kind(c, L.cin), tmp, c->stream))) return rc;
        src = tmp;
    }
    PMX_HIP(hipStreamSynchronize(c->stream));
    if (w_oihw) PMX_HIP(hipMemcpy(w_oihw, src, nw * sizeof(float), hipMemcpyDeviceToHost));
    if (bias) PMX_HIP(hipMemcpy(bias, src + nw, (size_t)L.cout * sizeof(float), hipMemcpyDeviceToHost));
    return PMX_OK;
}

extern "C" int pmx_train_get_state(pmx_ctx* c, const char* name, float* m_w, float* v_w, float* m_b, float* v_b, int* t)
{
    int rc, idx;
    if ((rc = tr_check(c, "pmx_train_get_state", true)) || (rc = state_layer(c, "pmx_train_get_state", name, &idx))) return rc;
    PMX_DEV(c);
    const LayerDesc& d = c->table[idx];
    const size_t nw = (size_t)d.cout * d.cin * d.ks * d.ks, off = c->bw.grad_off[idx];
    PMX_HIP(hipStreamSynchronize(c->stream));
    if (m_w) PMX_HIP(hipMemcpy(m_w, c->tr.m + off, nw * sizeof(float), hipMemcpyDeviceToHost));
    if (v_w) PMX_HIP(hipMemcpy(v_w, c->tr.v + off, nw * sizeof(float), hipMemcpyDeviceToHost));
    if (m_b) PMX_HIP(hipMemcpy(m_b, c->tr.m + off + nw, (size_t)d.cout * sizeof(float), hipMemcpyDeviceToHost));
    if (v_b) PMX_HIP(hipMemcpy(v_b, c->tr.v + off + nw, (size_t)d.cout * sizeof(float), hipMemcpyDeviceToHost));
    if (t) *t = c->tr.t[idx];
    return PMX_OK;
}

extern "C" int pmx_train_set_state(pmx_ctx* c, const char* name, const float* m_w, const float* v_w, const float* m_b, const float* v_b, int t)
{
    int rc, idx;
    if ((rc = tr_check(c, "pmx_train_set_state", true)) || (rc = state_layer(c, "pmx_train_set_state", name, &idx))) return rc;
    PMX_CHECK(m_w && v_w && m_b && v_b, PMX_ERR_INVALID, "pmx_train_set_state: null moments");
    PMX_CHECK(t >= 0, PMX_ERR_INVALID, "pmx_train_set_state: t = %d", t);
    PMX_DEV(c);
    const LayerDesc& d = c->table[idx];
    const size_t nw = (size_t)d.cout * d.cin * d.ks * d.ks, off = c->bw.grad_off[idx];
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(c->tr.m + off, m_w, nw * sizeof(float), hipMemcpyHostToDevice));
    PMX_HIP(hipMemcpy(c->tr.v + off, v_w, nw * sizeof(float), hipMemcpyHostToDevice));
    PMX_HIP(hipMemcpy(c->tr.m + off + nw, m_b, (size_t)d.cout * sizeof(float), hipMemcpyHostToDevice));
    PMX_HIP(hipMemcpy(c->tr.v + off + nw, v_b, (size_t)d.cout * sizeof(float), hipMemcpyHostToDevice));
    c->tr.t[idx] = t;
    return PMX_OK;
}

// which = 0 .. 6: pmx_get_pack's; 7: the f16 pack of the transposed layer (pmx_get_transposed_f16_pack)
static int get_pack(pmx_ctx* c, const char* name, int which, void* out, size_t cap_bytes, size_t* n_bytes)
{
    PMX_CHECK(c && name && n_bytes, PMX_ERR_INVALID, "pmx_get_pack: null arg");
    auto it = c->index.find(name);
    PMX_CHECK(it != c->index.end(), PMX_ERR_INVALID, "pmx_get_pack: unknown layer '%s'", name);
    const int idx = it->second;
    const PackedLayer* L = &c->layers[idx];
    if (which == 3 || which == 4 || which == 7) {
        PMX_CHECK((size_t)idx < c->bw.tl.size() && c->bw.tl[idx].set, PMX_ERR_STATE, "pmx_get_pack: layer '%s' has no transposed pack", name);
        L = &c->bw.tl[idx];
    }
    const DevBuf<uint16_t>& h = which == 5 || which == 7 ? L->d_w16 : L->d_w3;
    const DevBuf<float>& f = which == 0 || which == 3 ? L->d_w : which == 1 ? L->d_b : L->d_ww;
    const void* const b = which >= 5 ? (const void*)h.get() : (const void*)f.get();
    PMX_CHECK(L->set && b, PMX_ERR_STATE, "pmx_get_pack: pack %d of layer '%s' does not exist", which, name);
    *n_bytes = which >= 5 ? h.capacity() * sizeof(uint16_t) : f.capacity() * sizeof(float);
    PMX_CHECK(out && cap_bytes >= *n_bytes, PMX_ERR_CAPACITY, "pmx_get_pack: %zu bytes needed, %zu given", *n_bytes, cap_bytes);
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(out, b, *n_bytes, hipMemcpyDeviceToHost));
    return PMX_OK;
}

extern "C" int pmx_get_pack(pmx_ctx* c, const char* name, int which, void* out, size_t cap_bytes, size_t* n_bytes)
{
    PMX_CHECK(which >= 0 && which <= 6, PMX_ERR_INVALID, "pmx_get_pack: which = %d outside 0 .. 6", which);
    return get_pack(c, name, which, out, cap_bytes, n_bytes);
}

extern "C" int pmx_get_transposed_f16_pack(pmx_ctx* c, const char* name, void* out, size_t cap_bytes, size_t* n_bytes)
{
    return get_pack(c, name, 7, out, cap_bytes, n_bytes);
}

// test entry: the Adam launch on the caller's arrays (host, `total` floats each, updated in place); segment i covers floats
// [off[i], off[i] + n[i]), off[i] a multiple of 4, the segments in rising order and apart by whole 16-byte vectors
extern "C" int pmx_adam_apply(pmx_ctx* c, float* w, float* m, float* v, const float* grad, size_t total, const size_t* off, const unsigned* n,
                              const float* scale, const float* alpha_t, int nseg, float omb1, float omb2, float eps)
{
    PMX_CHECK(c && w && m && v && grad && off && n && scale && alpha_t, PMX_ERR_INVALID, "pmx_adam_apply: null arg");
    PMX_CHECK(nseg > 0 && nseg <= 4096, PMX_ERR_INVALID, "pmx_adam_apply: %d segments (1 .. 4096)", nseg);
    std::vector<AdamSeg> segs(nseg);
    unsigned blocks = 0;
    size_t end = 0;
    for (int i = 0; i < nseg; ++i) {
        PMX_CHECK(n[i] > 0 && off[i] % 4 == 0 && off[i] >= end && off[i] + ((size_t)n[i] + 3) / 4 * 4 <= total, PMX_ERR_INVALID,
                  "pmx_adam_apply: segment %d (offset %zu, %u floats) of %zu floats", i, off[i], n[i], total);
        end = off[i] + ((size_t)n[i] + 3) / 4 * 4;
        segs[i] = AdamSeg{(unsigned long long)off[i], n[i], blocks, scale[i], alpha_t[i]};
        blocks += (n[i] + ADAM_BLOCK_FLOATS - 1) / ADAM_BLOCK_FLOATS;
    }
    PMX_DEV(c);
    DevBuf<float> d[4];
    DevBuf<AdamSeg> ds;
    int rc;
    for (auto& b : d) if ((rc = b.alloc(total))) return rc;
    if ((rc = ds.alloc(nseg))) return rc;
    const float* src[4] = {w, m, v, grad};
    for (int i = 0; i < 4; ++i) PMX_HIP(hipMemcpy(d[i], src[i], total * sizeof(float), hipMemcpyHostToDevice));
    PMX_HIP(hipMemcpy(ds, segs.data(), nseg * sizeof(AdamSeg), hipMemcpyHostToDevice));
    rc = launch_adam(d[0], d[1], d[2], d[3], ds, nseg, blocks, omb1, omb2, eps, c->stream);
    PMX_HIP(hipStreamSynchronize(c->stream));
    if (rc) return rc;
    float* dst[3] = {w, m, v};
    for (int i = 0; i < 3; ++i) PMX_HIP(hipMemcpy(dst[i], d[i], total * sizeof(float), hipMemcpyDeviceToHost));
    return PMX_OK;
}
