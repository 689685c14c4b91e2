// pmx_api.hip -- C ABI of libpose_mi355x (include/pose_mi355x.h): context, weights, forward plan, accessors.
//
// Forward plan = models/CocoPoseNet.py:132-262 expressed as 47 convolution launches on NHWC buffers:
//   stem (12 launches; the three F.max_pooling_2d are fused into the epilogues of conv1_2, conv2_2, conv3_4),
//   stage 1 (5 launches) and stages 2-6 (7 launches each); the PAF branch (L1) and the heat-map branch (L2)
//   of a stage are the two groups (blockIdx.z) of one launch; F.concat (:168,...) is replaced by channel-slice
//   writes into the 192-channel "cat" buffer (layout in pmx_common.h).
#include "pmx_ctx.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <map>

// ------------------------------------------------------------------------------------------- errors
static thread_local char g_err[1024] = "";
void pmx_set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* pmx_last_error(void) { return g_err; }
extern "C" const char* pmx_version(void) { return "pose_mi355x 0.1 (gfx950, fp32 MFMA)"; }

extern "C" int pmx_device_count(int* n)
{
    PMX_CHECK(n, PMX_ERR_INVALID, "pmx_device_count: null");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
    *n = c;
    return PMX_OK;
}

// -------------------------------------------------------------------------------------- layer table

static int net_out_channels(int kind) { return kind == NET_FACE ? 71 : (kind == NET_HAND ? 22 : 19); }

// FaceNet / HandNet (models/FaceNet.py:12-75, models/HandNet.py): VGG-19 stem to conv5_2, conv5_3_CPM, single-branch 6-stage CPM
static std::vector<LayerDesc> make_cpm_table(int C)
{
    std::vector<LayerDesc> t = {
        {"conv1_1", 3, 64, 3}, {"conv1_2", 64, 64, 3}, {"conv2_1", 64, 128, 3}, {"conv2_2", 128, 128, 3},
        {"conv3_1", 128, 256, 3}, {"conv3_2", 256, 256, 3}, {"conv3_3", 256, 256, 3}, {"conv3_4", 256, 256, 3},
        {"conv4_1", 256, 512, 3}, {"conv4_2", 512, 512, 3}, {"conv4_3", 512, 512, 3}, {"conv4_4", 512, 512, 3},
        {"conv5_1", 512, 512, 3}, {"conv5_2", 512, 512, 3}, {"conv5_3_CPM", 512, 128, 3},
        {"conv6_1_CPM", 128, 512, 1}, {"conv6_2_CPM", 512, C, 1}};
    char buf[64];
    for (int s = 2; s <= 6; ++s) {
        snprintf(buf, sizeof buf, "Mconv1_stage%d", s); t.push_back({buf, C + 128, 128, 7});
        for (int i = 2; i <= 5; ++i) { snprintf(buf, sizeof buf, "Mconv%d_stage%d", i, s); t.push_back({buf, 128, 128, 7}); }
        snprintf(buf, sizeof buf, "Mconv6_stage%d", s); t.push_back({buf, 128, 128, 1});
        snprintf(buf, sizeof buf, "Mconv7_stage%d", s); t.push_back({buf, 128, C, 1});
    }
    return t;
}

static std::vector<LayerDesc> make_layer_table()   // models/CocoPoseNet.py:26-129
{
    std::vector<LayerDesc> t = {
        {"conv1_1", 3, 64, 3}, {"conv1_2", 64, 64, 3}, {"conv2_1", 64, 128, 3}, {"conv2_2", 128, 128, 3},
        {"conv3_1", 128, 256, 3}, {"conv3_2", 256, 256, 3}, {"conv3_3", 256, 256, 3}, {"conv3_4", 256, 256, 3},
        {"conv4_1", 256, 512, 3}, {"conv4_2", 512, 512, 3}, {"conv4_3_CPM", 512, 256, 3}, {"conv4_4_CPM", 256, 128, 3}};
    const char* br[2] = {"L1", "L2"};
    const int bco[2] = {38, 19};
    char buf[64];
    for (int g = 0; g < 2; ++g) {
        for (int i = 1; i <= 3; ++i) { snprintf(buf, sizeof buf, "conv5_%d_CPM_%s", i, br[g]); t.push_back({buf, 128, 128, 3}); }
        snprintf(buf, sizeof buf, "conv5_4_CPM_%s", br[g]); t.push_back({buf, 128, 512, 1});
        snprintf(buf, sizeof buf, "conv5_5_CPM_%s", br[g]); t.push_back({buf, 512, bco[g], 1});
    }
    for (int s = 2; s <= 6; ++s)
        for (int g = 0; g < 2; ++g) {
            snprintf(buf, sizeof buf, "Mconv1_stage%d_%s", s, br[g]); t.push_back({buf, 185, 128, 7});
            for (int i = 2; i <= 5; ++i) { snprintf(buf, sizeof buf, "Mconv%d_stage%d_%s", i, s, br[g]); t.push_back({buf, 128, 128, 7}); }
            snprintf(buf, sizeof buf, "Mconv6_stage%d_%s", s, br[g]); t.push_back({buf, 128, 128, 1});
            snprintf(buf, sizeof buf, "Mconv7_stage%d_%s", s, br[g]); t.push_back({buf, 128, bco[g], 1});
        }
    return t;
}



static int cout_pad_of(int cout) { return pmx_pk_cout_pad(cout); }

// the channel map of a layer's input (pack_index.h): the concat layers of the pose network (1) and of the face / hand networks (2 + C), else 0
int pmx_pack_kind(const pmx_ctx* c, int cin) { return c->kind == NET_POSE ? (cin == 185 ? 1 : 0) : cin == c->n_heat + 128 ? 2 + c->n_heat : 0; }

// ---- building packs: everything goes through the device packers (pmx_packs.hip); these calls return when the pack is complete ----------------
// host (w OIHW, bias or null) -> master (w | b) on the device, b zero without a bias; ordered before what `st` runs next
static int upload_master(float* master, const float* w, const float* bias, int cout, int cin, int ks, hipStream_t st)
{
    const size_t nw = (size_t)cout * cin * ks * ks;
    PMX_HIP(hipMemcpy(master, w, nw * sizeof(float), hipMemcpyHostToDevice));
    if (bias) PMX_HIP(hipMemcpy(master + nw, bias, (size_t)cout * sizeof(float), hipMemcpyHostToDevice));
    else PMX_HIP(hipMemsetAsync(master + nw, 0, (size_t)cout * sizeof(float), st));
    return PMX_OK;
}
// L (geometry filled) gets its direct pack and bias from master weights on the device; allocates what it does not hold
static int build_direct(PackedLayer& L, int kind, const float* master, hipStream_t st)
{
    int rc;
    if (!L.d_w && (rc = L.d_w.alloc((size_t)L.ks * L.ks * L.nch * L.cout_pad * CK))) return rc;
    if (!L.d_b && (rc = L.d_b.alloc((size_t)L.cout_pad))) return rc;
    if ((rc = pmx_pack_launch_one(PMX_PACK_DIRECT, pmx_pack_job_direct(master, L, kind), st))) return rc;
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
}
// P (geometry filled): the layer whose forward is the data gradient of the layer (cout, cin, ks, kind) with these master weights; no bias
static int build_transposed(PackedLayer& P, int cout, int cin, int ks, int kind, const float* master, hipStream_t st)
{
    int rc;
    if ((rc = P.d_w.alloc((size_t)ks * ks * P.nch * P.cout_pad * CK)) || (rc = P.d_b.alloc((size_t)P.cout_pad))) return rc;
    PMX_HIP(hipMemsetAsync(P.d_b, 0, (size_t)P.cout_pad * sizeof(float), st));
    if ((rc = pmx_pack_launch_one(PMX_PACK_TRANSPOSED, pmx_pack_job_transposed(master, cout, cin, ks, kind, P), st))) return rc;
    PMX_HIP(hipStreamSynchronize(st));
    return PMX_OK;
}

// the profile events of a launch are recorded on the stream of its call
static int prof_begin(pmx_ctx* c, const FwdCall& k, const std::string& name, double flops, double bytes, double issued = -1.0, bool record = true)
{
    if (!c->prof_on) return PMX_OK;
    int idx;
    auto it = c->prof_index.find(name);
    if (it == c->prof_index.end()) {
        idx = (int)c->prof.size();
        ProfEntry e; e.name = name; e.flops = flops; e.bytes = bytes; e.issued = issued < 0 ? flops : issued;
        c->prof.push_back(e);
        c->prof_index[name] = idx;
    } else idx = it->second;
    ProfPending p; p.entry = idx;
    for (Event* e : {&p.e0, &p.e1}) {
        if (!c->ev_pool.empty()) { *e = std::move(c->ev_pool.back()); c->ev_pool.pop_back(); }
        else if (int rc = e->create(hipEventDefault)) return rc;
    }
    if (record) PMX_HIP(hipEventRecord(p.e0, k.stream));
    c->pending.push_back(std::move(p));
    c->prof_open = (int)c->pending.size() - 1;
    return PMX_OK;
}
static int prof_end(pmx_ctx* c, const FwdCall& k)
{
    if (!c->prof_on || c->prof_open < 0) return PMX_OK;
    PMX_HIP(hipEventRecord(c->pending[c->prof_open].e1, k.stream));
    c->prof_open = -1;
    return PMX_OK;
}
// the profiler for the other translation units (pmx_boxes.hip): a labelled launch of `bytes` compulsory bytes
int pmx_prof_begin(pmx_ctx* c, const char* name, double bytes) { return c->prof_on == 1 ? prof_begin(c, pmx_call(c), name, 0, bytes) : PMX_OK; }
int pmx_prof_end(pmx_ctx* c) { return prof_end(c, pmx_call(c)); }
static int prof_collect(pmx_ctx* c)
{
    if (c->pending.empty()) return PMX_OK;
    PMX_HIP(hipStreamSynchronize(c->stream));
    for (auto& p : c->pending) {
        float ms = 0.f;
        PMX_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        c->prof[p.entry].total_ms += ms;
        c->prof[p.entry].launches += 1;
        c->ev_pool.push_back(std::move(p.e0));
        c->ev_pool.push_back(std::move(p.e1));
    }
    c->pending.clear();
    return PMX_OK;
}
static void pp_prof_cb(void* vc, const char* name, int begin)
{
    pmx_ctx* c = (pmx_ctx*)vc;
    if (begin) (void)prof_begin(c, pmx_call(c), std::string(name) + "|" + name, 0, 0);
    else (void)prof_end(c, pmx_call(c));
}


// Allocates the post-process arrays for B images at the capacities in p (cap_pk, cap_sub, cap_cand, cap_ppl): ONE allocation, `store`, with
// the arrays of the table below carved out of it at 256-byte-aligned offsets.  An array of no elements (the candidate store and the subset
// work table outside their large modes) stays null.  p.smoothed is not part of the set.
static int pp_alloc(PPBuffers& p, DevBuf<char>& store, size_t B)
{
    const size_t npk = (size_t)PMX_N_JOINTS * p.cap_pk, nl = PMX_N_LIMBS, ncn = nl * p.cap_pk, ncand = nl * p.cap_cand;
    p.rec_bytes = PMX_RECORD_BYTES(p.cap_ppl);
    p.scan_cap = p.cap_cand > PMX_LDS_CANDIDATES ? p.cap_cand : PMX_LDS_CANDIDATES;
    struct Part { void** q; size_t bytes; };
    auto part = [B](auto*& q, size_t per_image) { return Part{(void**)&q, B * per_image * sizeof(*q)}; };
    const Part parts[] = {
        part(p.pk_raw_key, npk), part(p.pk_raw_score, npk), part(p.pk_count, PMX_N_JOINTS), part(p.pk_x, npk), part(p.pk_y, npk),
        part(p.pk_score, npk), part(p.pk_start, PMX_N_JOINTS + 1), part(p.cn_a, ncn), part(p.cn_b, ncn), part(p.cn_score, ncn),
        part(p.cn_count, nl), part(p.cn_need, nl), part(p.scan_score, nl * p.scan_cap), part(p.scan_idx, nl * p.scan_cap), part(p.scan_cnt, nl),
        part(p.cand_score, ncand), part(p.cand_idx, ncand), part(p.cand_used, p.cap_cand > 0 ? 2 * ncn : 0),
        part(p.sub_work, p.cap_sub > PMX_LDS_SUBSETS ? (size_t)p.cap_sub * 20 : 0), part(p.subsets, (size_t)p.cap_sub * 20),
        part(p.status, 1), part(p.results, p.rec_bytes)};
    size_t total = 0;
    for (const Part& s : parts) total += pmx_align_up(s.bytes, 256);
    if (int rc = store.alloc(total)) return rc;
    size_t off = 0;
    for (const Part& s : parts) {
        *s.q = s.bytes ? store + off : nullptr;
        off += pmx_align_up(s.bytes, 256);
    }
    return PMX_OK;
}

extern "C" int pmx_create_net(pmx_ctx** out, const char* arch, int device, int max_batch, int max_h, int max_w);
extern "C" int pmx_create(pmx_ctx** out, int device, int max_batch, int max_h, int max_w)
{
    return pmx_create_net(out, "posenet", device, max_batch, max_h, max_w);
}

extern "C" int pmx_create_net(pmx_ctx** out, const char* arch, int device, int max_batch, int max_h, int max_w)
{
    PMX_CHECK(out && arch, PMX_ERR_INVALID, "pmx_create: null arg");
    *out = nullptr;
    int kind;
    if (!strcmp(arch, "posenet")) kind = NET_POSE;
    else if (!strcmp(arch, "facenet")) kind = NET_FACE;
    else if (!strcmp(arch, "handnet")) kind = NET_HAND;
    else { pmx_set_error("pmx_create_net: unknown arch '%s' (posenet | facenet | handnet)", arch); return PMX_ERR_INVALID; }
    PMX_CHECK(max_batch >= 1 && max_h >= 8 && max_w >= 8 && max_h % 8 == 0 && max_w % 8 == 0, PMX_ERR_INVALID,
              "pmx_create: max_batch >= 1 and max_h/max_w positive multiples of 8 required (got %d, %d, %d)", max_batch, max_h, max_w);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        pmx_set_error("pmx_create: no HIP device visible (this library has no CPU fallback)");
        return PMX_ERR_NO_DEVICE;
    }
    PMX_CHECK(device >= 0 && device < ndev, PMX_ERR_NO_DEVICE, "pmx_create: device %d out of range (%d devices)", device, ndev);
    hipDeviceProp_t prop;
    PMX_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        pmx_set_error("pmx_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
        return PMX_ERR_NO_DEVICE;
    }
    PMX_HIP(hipSetDevice(device));
    pmx_ctx* c = new pmx_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount;      // kernel / tile selection counts blocks against the CUs of this device
    c->max_batch = max_batch; c->max_h = max_h; c->max_w = max_w;
    c->kind = kind;
    c->n_heat = net_out_channels(kind);
    if (kind != NET_POSE) { c->cat_c = round_up(128 + c->n_heat, CK); c->cat_heat = 128; }
    c->table = kind == NET_POSE ? make_layer_table() : make_cpm_table(c->n_heat);
    c->layers.resize(c->table.size());
    for (size_t i = 0; i < c->table.size(); ++i) c->index[c->table[i].name] = (int)i;

    const size_t B = max_batch, HW = (size_t)max_h * max_w, hw8 = HW / 64;
    // any failure below frees what was created so far (the caller only ever sees a complete context or NULL)
    auto build = [&]() -> int {
        int rc;
        if ((rc = c->own_stream.create(hipStreamNonBlocking))) return rc;
        c->stream = c->own_stream;
        if ((rc = c->t0.create(hipEventDefault)) || (rc = c->t1.create(hipEventDefault))) return rc;
        if ((rc = c->in16.alloc(B * HW * PMX_IN_C))) return rc;
        if ((rc = c->act0.alloc(B * HW * 64))) return rc;      // conv1_1 out is the largest activation
        if ((rc = c->act1.alloc(B * HW * 16))) return rc;      // (H/2)(W/2) x 64 = (H/4)(W/4) x 256
        if ((rc = c->cat.alloc(B * hw8 * c->cat_c))) return rc;
        if ((rc = c->brA.alloc(B * hw8 * 256))) return rc;
        if ((rc = c->brB.alloc(B * hw8 * 256))) return rc;
        if ((rc = c->brT.alloc(B * hw8 * 1024))) return rc;
        PMX_HIP(hipMemsetAsync(c->cat, 0, B * hw8 * c->cat_c * sizeof(float), c->stream));   // pad channels stay zero forever (stream-ordered)
        if ((rc = c->nchw_tmp.alloc(B * HW * 3 < B * hw8 * 80 ? B * hw8 * 80 : B * HW * 3))) return rc;
        if ((rc = c->u8_tmp.alloc(B * HW * 3))) return rc;
        // post-process buffers at the initial capacities
        c->pp.cap_pk = PMX_INIT_PEAKS_PER_JOINT; c->pp.cap_sub = PMX_INIT_SUBSETS; c->pp.cap_ppl = PMX_INIT_PEOPLE; c->pp.cap_cand = 0;
        if ((rc = pp_alloc(c->pp, c->pp_store, B))) return rc;
        return c->d_scale.alloc(B * 2);
    };
    if (int rc = build()) { pmx_destroy(c); return rc; }

    // default Gaussian taps (sigma 2.5 -> radius 10); the Python binding overrides them with NumPy's values
    {
        const int r = (int)(4.0 * PMX_GAUSS_SIGMA + 0.5);
        std::vector<double> g(2 * r + 1);
        double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = -r; i <= r; ++i) g[i + r] = exp(-0.5 / (PMX_GAUSS_SIGMA * PMX_GAUSS_SIGMA) * (double)(i * i));
        // NumPy pairwise-sum order for n = 21: 8 running accumulators over the first 16, then the tail
        for (int j = 0; j < 8; ++j) acc[j] = g[j];
        for (int j = 0; j < 8; ++j) acc[j] += g[8 + j];
        double s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        for (int i = 16; i < 2 * r + 1; ++i) s += g[i];
        for (auto& v : g) v /= s;
        c->gauss = g;
    }
    *out = c;
    return PMX_OK;
}

extern "C" void pmx_destroy(pmx_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    // every buffer, event and stream of the context is a DevBuf, Event, Stream or Staging member and goes with it; the device is idle
    // after the synchronisation above, so the order in which the members go does not matter
    delete c;
}

extern "C" int pmx_set_stream(pmx_ctx* c, void* s)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    if (c->tr.on) {      // the lazy pack builders wait for the stream the training steps run on
        for (PackedLayer& l : c->layers) l.busy_stream = c->stream;
        for (PackedLayer& l : c->bw.tl) l.busy_stream = c->stream;
    }
    return PMX_OK;
}

extern "C" int pmx_synchronize(pmx_ctx* c)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_set_option(pmx_ctx* c, const char* key, int value)
{
    PMX_CHECK(c && key, PMX_ERR_INVALID, "null arg");
    c->opt_epoch += 1;
    if (!strcmp(key, "force_variant_k7")) c->opt_force[7] = value;
    else if (!strcmp(key, "force_variant_k3")) c->opt_force[3] = value;
    else if (!strcmp(key, "force_variant_k1")) c->opt_force[1] = value;
    else if (!strcmp(key, "keep_smoothed")) c->opt_keep_smoothed = value;
    else if (!strcmp(key, "stop_stage")) c->opt_stop_stage = value;
    else if (!strcmp(key, "kernel_gen")) c->opt_kernel_gen = value;
    else if (!strcmp(key, "fuse_pairs")) c->opt_fuse_pairs = value;
    else if (!strcmp(key, "fuse_conv1")) c->opt_fuse_conv1 = value;
    else if (!strcmp(key, "conv1_wino")) c->opt_conv1_wino = value;
    else if (!strcmp(key, "precise_lanes")) c->opt_precise_lanes = value < 1 ? 1 : (value > PMX_PR_LANES ? PMX_PR_LANES : value);
    else if (!strcmp(key, "precise_plain")) c->opt_precise_plain = value;
    else if (!strcmp(key, "precise_lane_priority")) c->opt_precise_lane_priority = value != 0;
    else if (!strcmp(key, "precise_table_cap")) c->opt_precise_table_cap = value < 1 ? 1 : value;
    else if (!strcmp(key, "cubic_rows")) c->opt_cubic_rows = value;
    else if (!strcmp(key, "precision")) {
        PMX_CHECK(value >= 0 && value <= 2, PMX_ERR_INVALID,
                  "pmx_set_option: \"precision\" = %d: 0 (fp32), 1 (bf16x3, opt-in build) or 2 (f16 mode)", value);
        PMX_CHECK(value != 1 || conv_bf16x3_launch != nullptr, PMX_ERR_INVALID,
                  "pmx_set_option: \"precision\" = %d needs the opt-in bf16x3 kernels, which this build does not carry (rebuild with PMX_BUILD_BF16X3=1)", value);
        c->opt_precision = value;
    }
    else if (!strcmp(key, "f16_bn")) {
        PMX_CHECK(value == 0 || value == 64 || value == 128, PMX_ERR_INVALID,
                  "pmx_set_option: \"f16_bn\" = %d: 0 (the launch-size rule), 64 or 128 output channels per block", value);
        c->opt_f16_bn = value;
    }
    else if (!strcmp(key, "conv_algo")) c->opt_conv_algo = value;
    else if (!strcmp(key, "wino_min_fill")) c->opt_wino_min_fill = value;
    else if (!strcmp(key, "wino_unit_eff")) c->opt_wino_unit_eff = value;
    else if (!strcmp(key, "wino_geom")) c->opt_wino_geom = value;
    else if (!strcmp(key, "wino_tail")) c->opt_wino_tail = value;
    else if (!strcmp(key, "wino_tail_g")) c->opt_wino_tail_g = value;
    else if (!strcmp(key, "wino_unit_g")) c->opt_wino_unit_g = value;
    else if (!strcmp(key, "wino_split")) c->opt_wino_split = value;
    else if (!strcmp(key, "wino_tail_merge")) c->opt_wino_tail_merge = value;
    else if (!strcmp(key, "batch_chains")) {
        PMX_CHECK(value >= -1 && value <= 1, PMX_ERR_INVALID, "pmx_set_option: \"batch_chains\" = %d: 0 (off), 1 (wherever the plans allow) or -1 (automatic)", value);
        c->opt_batch_chains = value;
    }
    else if (!strcmp(key, "ksplit")) c->opt_ksplit = value;
    else if (!strcmp(key, "ksplit_plan")) c->opt_ksplit = value > 0 ? -value : 0;     // decimal digits = chunks per slice, e.g. 3221
    else if (!strcmp(key, "conv_min_lds")) c->opt_conv_min_lds = value;
    else if (!strcmp(key, "conv_v5_lds")) c->opt_conv_v5_lds = value;
    else if (!strcmp(key, "pp_generic")) c->opt_pp_generic = value;
    else if (!strcmp(key, "pp_limbs_slices")) c->opt_limbs_slices = value;
    else if (!strcmp(key, "peaks_gpu_branch")) { c->opt_gpu_branch_peaks = value; c->tab_in_h = -1; }
    else if (!strcmp(key, "kp_flip_x")) c->opt_kp_flip_x = value != 0;
    else if (!strcmp(key, "wgrad_strips")) c->opt_wgrad_strips = value;
    else if (!strcmp(key, "grad_precision")) {
        PMX_CHECK(value == 0 || value == 2, PMX_ERR_INVALID,
                  "pmx_set_option: \"grad_precision\" = %d: 0 (fp32 gradients) or 2 (f16 operands, fp32 sums: the 3x3 / 7x7 layers of "
                  "pmx_conv2d_backward and pmx_backward_head)", value);
        c->opt_grad_precision = value;
    }
    else if (!strcmp(key, "loss_scale_log2")) {
        PMX_CHECK(value >= 0 && value <= 24, PMX_ERR_INVALID,
                  "pmx_set_option: \"loss_scale_log2\" = %d: k = 0 .. 24, the loss gradients of the next hooked forward times 2^k", value);
        c->opt_loss_scale_log2 = value;
    }
    else if (!strcmp(key, "trunk_keep_g")) c->opt_trunk_keep_g = value != 0;
    else { pmx_set_error("pmx_set_option: unknown key '%s'", key); return PMX_ERR_INVALID; }
    return PMX_OK;
}

// ------------------------------------------------------------------------------------------ weights
extern "C" int pmx_set_layer(pmx_ctx* c, const char* name, const float* w, const float* bias, int cout, int cin, int ks)
{
    PMX_CHECK(c && name && w, PMX_ERR_INVALID, "pmx_set_layer: null arg");
    PMX_DEV(c);
    auto it = c->index.find(name);
    PMX_CHECK(it != c->index.end(), PMX_ERR_WEIGHTS, "pmx_set_layer: unknown layer '%s'", name);
    const LayerDesc& d = c->table[it->second];
    PMX_CHECK(d.cin == cin && d.cout == cout && d.ks == ks, PMX_ERR_WEIGHTS,
              "pmx_set_layer: '%s' expects (cout %d, cin %d, k %d), got (%d, %d, %d)", name, d.cout, d.cin, d.ks, cout, cin, ks);
    PackedLayer& L = c->layers[it->second];
    const int kind = pmx_pack_kind(c, cin);
    PMX_HIP(hipStreamSynchronize(c->stream));     // layer may be in use by queued work
    // (w | b) goes up once: into the layer's master segment while training is on (the next step packs from there), else into a staging buffer
    int rc;
    DevBuf<float> staging;
    float* master = pmx_train_master(c, it->second);
    if (master) { L.busy = true; L.busy_stream = c->stream; }
    else {
        if ((rc = staging.alloc((size_t)cout * cin * ks * ks + cout))) return rc;
        master = staging;
    }
    if ((rc = upload_master(master, w, bias, cout, cin, ks, c->stream))) return rc;
    pmx_layer_geometry(L, cout, cin, ks, pmx_pk_cin_pad(kind, cin));
    if ((rc = build_direct(L, kind, master, c->stream))) return rc;
    // the bf16x3 pack (1.5x the fp32 weights) and the Winograd pack (16/9 x for 3x3, 81/49 x for 7x7) are derived from the packed fp32
    // weights on first use (ensure_*_pack): a context that never runs those kernels neither holds nor computes them
    L.d_w3.reset(); L.d_w16.reset(); L.d_ww.reset();
    if ((size_t)it->second < c->bw.tl.size()) c->bw.tl[it->second] = PackedLayer();      // the data-gradient pack of the old weights
    L.set = true;
    return PMX_OK;
}

extern "C" int pmx_weights_missing(pmx_ctx* c, int* n)
{
    PMX_CHECK(c && n, PMX_ERR_INVALID, "null arg");
    int m = 0;
    for (auto& l : c->layers) m += l.set ? 0 : 1;
    *n = m;
    return PMX_OK;
}

// ------------------------------------------------------------------------------------------ forward
// Derived weight packs -- Winograd, f16, bf16x3, conv1_1's fused-kernel pack (which lives in conv1_1's otherwise unused Winograd slot) --
// are built on the device from the direct pack when a kernel first needs them: allocate, launch the kind's packer for job `j` on the
// stream of the call that needs it, wait for it.  The slot takes the buffer only when it is complete: a failure leaves no pointer to garbage
// behind, and the lanes of detect_precise may share the pack from their own streams as soon as this returns.
template <typename T>
static int derive_on_device(hipStream_t st, const PackedLayer& L, int kind, DevBuf<T>& slot, PackJob j)
{
    if (slot) return PMX_OK;
    if (L.busy) PMX_HIP(hipStreamSynchronize(L.busy_stream));      // a training step may still be writing d_w
    DevBuf<T> d;
    int rc;
    if ((rc = d.alloc(j.total))) return rc;
    j.dst = d.get();
    if ((rc = pmx_pack_launch_one(kind, j, st))) return rc;
    PMX_HIP(hipStreamSynchronize(st));
    slot = std::move(d);
    return PMX_OK;
}
static int ensure_wino_pack(hipStream_t st, PackedLayer& L) { return derive_on_device(st, L, PMX_PACK_WINO, L.d_ww, pmx_pack_job_wino(L, nullptr)); }
static int ensure_conv1_pack(hipStream_t st, PackedLayer& L) { return derive_on_device(st, L, PMX_PACK_CONV1, L.d_ww, pmx_pack_job_conv1(L, nullptr)); }
static int ensure_bf16x3_pack(hipStream_t st, PackedLayer& L) { return derive_on_device(st, L, PMX_PACK_BF16X3, L.d_w3, pmx_pack_job_bf16x3(L, nullptr)); }
// the f16 pack (half the fp32 weights' bytes): every 3x3 / 7x7 layer in f16 mode
static int ensure_f16_pack(hipStream_t st, PackedLayer& L) { return derive_on_device(st, L, PMX_PACK_F16, L.d_w16, pmx_pack_job_f16(L, nullptr)); }

// Launches one convolution (1 or 2 groups) whose ConvArgs describe the FINAL result (real bias, ReLU, pool, output slices).
// With S > 1 K slices the slice blocks write raw partial sums into the slab scratch of the call's working set and conv_splitk_reduce
// produces the final result (slabs added in slice order, then bias, ReLU, pool).
static const int SK_ZERO_BIAS = PMX_SK_ZERO_BIAS;
// the slab scratch at `need` floats at least, and the zero bias vector of the slice blocks (made on first use)
// (the second of two half-batch chains has both to itself: k.scratch)
static DevBuf<float>& sk_slabs(const FwdCall& k) { return k.scratch ? k.scratch->sk_scratch : k.ws.sk_scratch; }
static DevBuf<float>& sk_zeros(pmx_ctx* c, const FwdCall& k) { return k.scratch ? k.scratch->sk_zero_bias : c->sk_zero_bias; }
static int sk_reserve(pmx_ctx* c, const FwdCall& k, size_t need)
{
    int rc;
    if ((rc = sk_slabs(k).ensure(need, k.stream))) return rc;
    DevBuf<float>& zero = sk_zeros(c, k);
    if (!zero) {
        if ((rc = zero.alloc(SK_ZERO_BIAS))) return rc;
        // stream-ordered: a null-stream hipMemset is not ordered against this (non-blocking) stream and may still be in flight
        // when the first slice kernel reads the vector
        PMX_HIP(hipMemsetAsync(zero, 0, SK_ZERO_BIAS * sizeof(float), k.stream));
    }
    return PMX_OK;
}
// The slab form of a launch (K slices, Winograd units): S x groups slabs of `slab` floats in the scratch.  `a` (a copy of a0) is pointed at
// them -- raw sums of all cout_pad columns: zero bias, no ReLU, no pool -- and `r`, the arguments of the kernel that adds the slabs of a
// group (r.slabs[]), takes over what a0 says about the final result; its slab count and whatever else is its own are the caller's.
template <typename Reduce>
static int slab_redirect(pmx_ctx* c, const FwdCall& k, const ConvArgs& a0, int groups, int S, size_t slab, unsigned long long kbounds, ConvArgs& a, Reduce& r)
{
    PMX_CHECK(a0.cout_pad <= SK_ZERO_BIAS, PMX_ERR_INVALID, "split-K: cout_pad %d too large", a0.cout_pad);
    if (int rc = sk_reserve(c, k, slab * S * groups)) return rc;
    memset(&r, 0, sizeof r);
    for (int g = 0; g < groups; ++g) {
        float* base = sk_slabs(k) + (size_t)g * S * slab;
        r.slabs[g] = base; r.bias[g] = a0.g[g].bias; r.out[g] = a0.g[g].out; r.cout[g] = a0.g[g].cout;
        a.g[g].out = base; a.g[g].bias = sk_zeros(c, k); a.g[g].cout = a0.cout_pad;
    }
    a.ldc = a0.cout_pad; a.relu = 0; a.pool = 0; a.ksplit = S; a.slab_stride = (long long)slab; a.kbounds = kbounds;
    r.slab_stride = (long long)slab; r.B = a0.B; r.H = a0.H; r.W = a0.W; r.ld_slab = a0.cout_pad; r.ldc = a0.ldc;
    r.relu = a0.relu; r.pool = a0.pool;
    return PMX_OK;
}
static int launch_conv(pmx_ctx* c, const FwdCall& k, const ConvArgs& a0, int groups, int v, const SplitPlan& plan)
{
    ConvArgs a = a0;
    if (plan.S <= 1) {
        a.ksplit = 1; a.slab_stride = 0;
        return conv_launch(v, a, groups, c->opt_conv_min_lds, c->opt_conv_v5_lds, k.stream);
    }
    SplitKReduceArgs r;
    int rc = slab_redirect(c, k, a0, groups, plan.S, (size_t)a0.B * a0.H * a0.W * a0.cout_pad, plan.bounds, a, r);
    if (rc) return rc;
    r.ksplit = plan.S;
    if ((rc = conv_launch(v, a, groups, c->opt_conv_min_lds, c->opt_conv_v5_lds, k.stream))) return rc;
    return conv_splitk_reduce(r, groups, k.stream);
}

// Unit mode of the Winograd kernel (single images): a (tile, group) is cut into S units -- pass 1 over g chunks each (ceil(nch / g) units)
// and, for 7x7, row 6, column 6 and tap (6, 6) -- that run as separate blocks writing slabs, combined in unit order by the split-K combine kernel
// (bias, ReLU, pool there)
static int launch_wino_units(pmx_ctx* c, const FwdCall& k, const ConvArgs& a0, int ks, int groups, int g)
{
    const int S = (a0.nch + g - 1) / g + (ks == 7 ? 3 : 0);
    PMX_CHECK(S >= 2 && S <= 8, PMX_ERR_INVALID, "winograd units: %d slabs", S);
    ConvArgs a = a0;
    SplitKReduceArgs r;
    int rc = slab_redirect(c, k, a0, groups, S, (size_t)a0.B * a0.H * a0.W * a0.cout_pad, (unsigned long long)g, a, r);
    if (rc) return rc;
    r.ksplit = S;
    if ((rc = conv_wino_launch(a, ks, groups, k.stream))) return rc;
    return conv_splitk_reduce(r, groups, k.stream);
}

// profile entry of a layer's launch.  suffix: "@<first image>+<count>" on a part of a batch cut by images (run_conv, for_each_part), the
// last thing of every label of the launch
struct ConvProf {
    std::string name; double flops, bytes, issued; std::string suffix;
    std::string label(const char* part = "") const { return name + part + suffix; }
};
// the tails of all images of the launch as one stream of tiles, 32 per block (conv_wino_kernel<KS, 0, 1, 3>)?
static bool wino_tail_merged(const pmx_ctx* c, const ConvArgs& a)
{
    return c->opt_wino_tail_merge != 0 && wino_tail_mergeable(a.B, a.H, a.W, a.lda);
}
// Run geometry of the Winograd kernel (46-pixel-wide maps): the full blocks [0, nfull) of every image as one plain launch; the part-filled
// last block of every image in unit mode (S units of g pass-1 chunks (+ row 6, column 6, tap (6, 6)) writing compact slabs) + the combine
// kernel.  B = 32 at 46 x 46: 16 x 32 x 2 = 1024 full blocks = exactly 4 rounds of the 256 CUs, then 64 x 7 short unit blocks, instead of
// 5 rounds of 18 x 32 x 2 rectangles.  tail_g = 0: every block (also the part-filled one) in the plain launch.
static int launch_wino_run(pmx_ctx* c, const FwdCall& k, const ConvArgs& a0, int ks, int groups, int tail_g, const ConvProf* pf)      // (pf null: not profiled)
{
    const int ntiles = PMX_WINO_RUN_TX * ((a0.H + 1) / 2), nblk = (ntiles + PMX_WINO_RUN_TILES - 1) / PMX_WINO_RUN_TILES, nfull = ntiles / PMX_WINO_RUN_TILES;
    ConvArgs a = a0;
    a.ksplit = 1; a.slab_stride = 0; a.run_j0 = 0; a.run_nb = tail_g ? nfull : nblk;
    // profile: the three launches of a layer with a unit-mode tail are separate entries -- "<layer>|<kernel>" (the full blocks; carries
    // their share of the FLOP), "...:units", "...:combine" -- so that each can be held against its own rocprofv3 kernel row
    const double share = tail_g ? (double)nfull * PMX_WINO_RUN_TILES / ntiles : 1.0;
    int rc;
    if (pf && c->prof_on == 2) {
        // inside timed regions: the dispatch stamps the two events itself (no hipEventRecord barrier packets around the launch)
        if ((rc = prof_begin(c, k, pf->label(), pf->flops * share, pf->bytes, pf->issued * share, /*record=*/false))) return rc;
        c->prof_open = -1;
        rc = conv_wino_run_launch(a, ks, groups, k.stream, c->pending.back().e0, c->pending.back().e1);
        if (rc) {       // nothing was dispatched, so nothing will ever stamp the pair: take it back (prof_collect would fail on it for good)
            c->ev_pool.push_back(std::move(c->pending.back().e0));
            c->ev_pool.push_back(std::move(c->pending.back().e1));
            c->pending.pop_back();
        }
    } else {
        if (pf && (rc = prof_begin(c, k, pf->label(), pf->flops * share, pf->bytes, pf->issued * share))) return rc;
        rc = conv_wino_run_launch(a, ks, groups, k.stream);
        if (pf && !rc) rc = prof_end(c, k);
    }
    if (rc || !tail_g) return rc;
    PMX_CHECK(nfull >= 1 && nfull < nblk, PMX_ERR_INVALID, "winograd tail: no part-filled block (%d tiles)", ntiles);
    const int S = (a0.nch + tail_g - 1) / tail_g + (ks == 7 ? 3 : 0);
    PMX_CHECK(S >= 2 && S <= 8, PMX_ERR_INVALID, "winograd tail: %d slabs", S);
    const int nslab = a0.W / (2 * PMX_WINO_RUN_TX);
    // merged: the tails of all images as one stream of tiles, 32 per block (46 x 46: 17 tiles per image -- every MFMA row a real tile)
    const bool merged = wino_tail_merged(c, a0);
    const size_t slab = merged ? (size_t)wino_tail_merged_blocks(a0.B, a0.H) * PMX_WINO_RUN_TILES * 4 * a0.cout_pad      // [block of the stream][tile][pixel][cout_pad]
                               : (size_t)a0.B * nslab * PMX_WINO_RUN_TILES * 4 * a0.cout_pad;      // one block per (image, slab): [image][slab][tile][pixel][cout_pad]
    WinoTailReduceArgs r;
    if ((rc = slab_redirect(c, k, a0, groups, S, slab, (unsigned long long)tail_g, a, r))) return rc;
    a.run_j0 = nfull; a.run_nb = 1;
    r.S = S; r.run_j0 = nfull; r.run_nb = 1; r.nslab = nslab; r.merged = merged;
    // (profile mode 2 -- the dominant kernel only, inside timed regions -- leaves these two short launches without events: an event pair
    //  costs ~5 us of idle stream)
    const bool pf_all = pf && c->prof_on == 1;
    if (pf_all && (rc = prof_begin(c, k, pf->label(":units"), pf->flops * (1.0 - share), 0.0, pf->issued * (1.0 - share)))) return rc;
    if ((rc = merged ? conv_wino_merged_tail_launch(a, ks, groups, k.stream) : conv_wino_run_launch(a, ks, groups, k.stream))) return rc;
    if (pf_all && (rc = prof_end(c, k))) return rc;
    if (pf_all && (rc = prof_begin(c, k, pf->label(":combine"), 0.0, 0.0, 0.0))) return rc;
    if ((rc = conv_wino_tail_reduce(r, groups, k.stream))) return rc;
    return pf_all ? prof_end(c, k) : PMX_OK;
}

// the context options, and the call's "conv_algo", the choice of a 3x3 / 7x7 layer's form depends on (conv_select.hip)
static WinoSelectOpts wino_opts(const pmx_ctx* c, const FwdCall& k, int ks, int groups, int lda)
{
    WinoSelectOpts o;
    o.conv_algo = k.conv_algo; o.precision = k.precision; o.forced_variant = c->opt_force[ks]; o.ksplit = c->opt_ksplit;
    o.wino_unit_eff = c->opt_wino_unit_eff; o.wino_min_fill = c->opt_wino_min_fill; o.wino_geom = c->opt_wino_geom; o.wino_tail = c->opt_wino_tail;
    o.wino_tail_g = c->opt_wino_tail_g; o.wino_tail_merge = c->opt_wino_tail_merge; o.groups = groups; o.lda = lda; o.wino_unit_g = c->opt_wino_unit_g;
    o.wino_split = c->opt_wino_split; o.ncu = c->num_cus;
    return o;
}
// every group of the launch has a Winograd form, and the groups agree in what the launch shares?
static bool wino_layers_ok(const PackedLayer* L0, const PackedLayer* L1)
{
    return wino_eligible(L0->ks, L0->cin_pad, L0->cout_pad) && (!L1 || (wino_eligible(L1->ks, L1->cin_pad, L1->cout_pad) && L1->cout == L0->cout));
}

// What one convolution launch (1 or 2 groups of the same geometry) will do: the ONE place that knows which kernel form a layer shape takes
// under the context options and which weight pack that form reads.  The network (run_conv) and the single-layer entry (pmx_conv2d) both
// plan, then launch.
//   FORM_DIRECT      the direct kernels: `variant` (+ its bf16x3 twin with option "precision" = 1), `split` = the K slices
//   FORM_WINO        the Winograd kernel on 8 x 16 rectangles (a heterogeneous forward: over the segment table of the level)
//   FORM_WINO_RUN    ... in the run geometry; tail_g > 0: the part-filled last blocks in unit mode, tail_g chunks per pass-1 unit
//   FORM_WINO_UNITS  ... in unit mode, unit_g chunks per pass-1 unit
//   FORM_F16         f16 mode (the call's precision = 2): a 3x3 / 7x7 layer as ONE conv_f16_kernel launch, whatever the batch (no Winograd, no
//                    split-K, no cut by images: the per-output summation order must not depend on the launch)
enum ConvForm { FORM_DIRECT, FORM_WINO, FORM_WINO_RUN, FORM_WINO_UNITS, FORM_F16 };
struct ConvPlan {
    ConvForm form = FORM_DIRECT;
    ConvIO io;                       // what the caller said (launch_plan_chains slices it by images)
    ConvArgs a;                      // the FINAL result (real bias, ReLU, pool, output slices), weights = the pack of the form
    int ks = 0, groups = 1, variant = 0, unit_g = 0, tail_g = 0;
    SplitPlan split{};
    bool prof = false;               // profiled under c->prof_on (never without a label)
    ConvProf pf;
};

// what `io` says, in the launch arguments (the weights, and whatever else the kernel form decides, are the caller's)
static void args_io(ConvArgs& a, const ConvIO& io)
{
    a.B = io.B; a.H = io.H; a.W = io.W; a.lda = io.lda; a.ldc = io.ldc; a.relu = io.relu; a.pool = io.pool;
    for (int g = 0; g < 2; ++g) { a.g[g].in = io.in[g]; a.g[g].out = io.out[g]; }
}

// L1 null: one group (io.in[1], io.out[1] unused); label null: never profiled.  Makes sure the derived pack of the form exists.
static int plan_conv(pmx_ctx* c, const FwdCall& k, ConvPlan& p, const char* label, PackedLayer* L0, PackedLayer* L1, const ConvIO& io)
{
    const PackedLayer& L = *L0;
    const int ks = L.ks, groups = L1 ? 2 : 1;
    const int lda = io.lda, ldc = io.ldc, B = io.B, H = io.H, W = io.W, pool = io.pool, level = io.level;
    const char* who = label ? label : "pmx_conv2d";
    const bool seg = k.seg && level >= 0;
    const double npix = seg ? (double)k.seg->pix[level] : (double)B * H * W;
    PackedLayer* const Lg[2] = {L0, L1};
    auto ensure = [&](int (*fn)(hipStream_t, PackedLayer&)) { const int rc = fn(k.stream, *L0); return rc || !L1 ? rc : fn(k.stream, *L1); };
    p.ks = ks; p.groups = groups; p.io = io;
    p.prof = label && (c->prof_on == 1 || (c->prof_on == 2 && ks == 7));
    ConvArgs& a = p.a;
    memset(&a, 0, sizeof a);
    args_io(a, io);
    a.nch = L.nch; a.cout_pad = L.cout_pad;
    double flops = 0;
    for (int g = 0; g < groups; ++g) {
        const PackedLayer& G = *Lg[g];
        a.g[g].w = G.d_w; a.g[g].bias = G.d_b; a.g[g].cout = G.cout;
        flops += 2.0 * npix * (double)G.cout * G.cin * G.ks * G.ks;
    }
    int rc;
    const int precision = k.precision;       // the call's, not the context's: pmx_conv2d_backward plans z and dx under different ones
    if (precision == 2 && ks > 1) {
        p.form = FORM_F16;
        PMX_CHECK(!k.seg || seg, PMX_ERR_INVALID, "heterogeneous forward: layer %s without a resolution level", who);
        PMX_CHECK(!L1 || (L1->ks == ks && L1->nch == L.nch && L1->cout_pad == L.cout_pad), PMX_ERR_INVALID, "conv f16: the two groups of %s differ in shape", who);
        if ((rc = ensure(ensure_f16_pack))) return rc;
        for (int g = 0; g < groups; ++g) a.g[g].w = (const float*)Lg[g]->d_w16.get();
    } else if (seg) {
        // heterogeneous launch: the plain Winograd kernel on 8 x 16 rectangles over all segments (every 3x3 / 7x7 layer of the pose network
        // qualifies; its per-pixel arithmetic is that of a plain launch of each image alone -- oracle/conv_fma_ref::conv_wino)
        PMX_CHECK(wino_layers_ok(L0, L1) && (precision == 0 || precision == 2), PMX_ERR_INVALID,
                  "heterogeneous forward: layer %s has no Winograd form", who);
        p.form = FORM_WINO;
    } else {
        p.variant = conv_pick_variant(ks, L.cout_pad, H, W, B * groups, c->opt_force[ks], c->opt_kernel_gen, pool, groups == 1 ? L.cin : 9999,
                                      precision == 1 && ks > 1, c->num_cus);
        if (precision == 1 && ks > 1 && conv_bf16x3_twin(p.variant) >= 0) {
            if ((rc = ensure(ensure_bf16x3_pack))) return rc;
            p.variant = conv_bf16x3_twin(p.variant);
            for (int g = 0; g < groups; ++g) a.g[g].w = (const float*)Lg[g]->d_w3.get();
        }
        int wrun = 0;
        const int wmode = wino_layers_ok(L0, L1) ? wino_select(wino_opts(c, k, ks, groups, lda), ks, L.cin_pad, L.cout_pad, L.cout, ldc, B * groups, H, W,
                                                               pool, &p.unit_g, &wrun, &p.tail_g) : 0;
        p.form = wmode == 2 ? FORM_WINO_UNITS : wmode == 1 ? (wrun ? FORM_WINO_RUN : FORM_WINO) : FORM_DIRECT;
    }
    const bool wino = p.form == FORM_WINO || p.form == FORM_WINO_RUN || p.form == FORM_WINO_UNITS;
    if (wino) {
        if ((rc = ensure(ensure_wino_pack))) return rc;
        a.nch = L.cin_pad / 32;
        for (int g = 0; g < groups; ++g) a.g[g].w = Lg[g]->d_ww;
    }
    if (seg) {
        const int t = PMX_SEG_RECT(level, pool);
        a.nseg = (int)k.seg->segs.size(); a.segs = k.seg->table(t); a.seg_tiles = k.seg->tiles[t];
    }
    if (p.form == FORM_DIRECT) {
        p.split = conv_pick_ksplit(p.variant, H, W, B, groups, L.cout_pad, L.nch, pool, c->opt_ksplit, c->num_cus);
        if (L.cout % 4 != 0 || ldc % 4 != 0 || (L1 && L1->cout != L.cout)) p.split.S = 1;
    }
    if (!p.prof) return PMX_OK;
    // the profile entry: "<layer>|<kernel><what the form adds>", algorithmic FLOP, compulsory bytes (a whole launch in unit mode is
    // entered without the pool's share), FLOP issued to the matrix cores
    std::string kn;
    double issued = flops;
    if (p.form == FORM_F16) {
        kn = ks == 7 ? "conv_f16_7x7" : "conv_f16_3x3";
        // issued: every MFMA of the launch -- the tile padding of the map edges, the channel padding of cin and of the block's BN columns
        const long long tiles = conv_f16_tiles(a);
        const int bn = conv_f16_bn(a, groups, c->opt_f16_bn, c->num_cus);
        issued = 2.0 * (double)tiles * 128.0 * (double)round_up(L.cout, bn) * (L.nch * CK) * ks * ks * groups;
    } else if (wino) {
        kn = ks == 7 ? "conv_wino_f2x2_7x7" : "conv_wino_f2x2_3x3";
        // "r": run geometry; "/t<g>": its part-filled last blocks in unit mode, g chunks per pass-1 unit (part of the arithmetic), "m": merged tails
        if (seg) kn += "/seg";
        if (p.form == FORM_WINO_UNITS) kn += "/u" + std::to_string(p.unit_g);
        if (p.form == FORM_WINO_RUN) kn += "r";
        if (p.tail_g) kn += "/t" + std::to_string(p.tail_g) + (p.form == FORM_WINO_RUN && wino_tail_merged(c, a) ? "m" : "");
        // products per 2 x 2 output tile and channel pair: 3x3: 16 of 36; 7x7: 4 x 16 + 4 x 8 + 4 = 100 of 196
        issued = flops * (ks == 7 ? 100.0 / 196.0 : 16.0 / 36.0);
    } else {
        kn = conv_variant(p.variant).name;
        if (p.split.S > 1) {       // "/k<chunks of slice 0>-<slice 1>-...": the K slices (+ the combine kernel) are part of the launch
            kn += "/k";
            for (int i = 0; i < p.split.S; ++i) kn += (i ? "-" : "") + std::to_string(p.split.sizes[i]);
        }
    }
    const double bytes = 4.0 * npix * ((double)L.cin * groups + (double)L.cout * groups / (pool && p.form != FORM_WINO_UNITS ? 4 : 1));
    p.pf = ConvProf{std::string(label) + "|" + kn, flops, bytes, issued};
    return PMX_OK;
}

// profile begin, the launch sequence of the plan's form, profile end
static int launch_plan(pmx_ctx* c, const FwdCall& k, const ConvPlan& p)
{
    const ConvProf* pf = p.prof ? &p.pf : nullptr;
    if (p.form == FORM_WINO_RUN) return launch_wino_run(c, k, p.a, p.ks, p.groups, p.tail_g, pf);      // (up to three launches, an entry each)
    int rc;
    if (pf && (rc = prof_begin(c, k, pf->label(), pf->flops, pf->bytes, pf->issued))) return rc;
    switch (p.form) {
    case FORM_F16: rc = conv_f16_launch(p.ks, p.a, p.groups, c->opt_f16_bn, c->num_cus, k.stream); break;
    case FORM_WINO_UNITS: rc = launch_wino_units(c, k, p.a, p.ks, p.groups, p.unit_g); break;
    case FORM_WINO: rc = conv_wino_launch(p.a, p.ks, p.groups, k.stream); break;
    default: rc = launch_conv(c, k, p.a, p.groups, p.variant, p.split); break;
    }
    if (rc) return rc;
    return pf ? prof_end(c, k) : PMX_OK;
}

// ---- the parts of a launch: images [first, first + n) of its B ----
// One part, the launch itself, unless the forward runs as two half-batch chains (pmx_ctx.h: BatchChain, ChainSplit): then the images of each
// chain, on the chain's call.  `share` = n / B scales the profile figures of the whole launch, `suffix` ends the part's profile labels.
struct LaunchPart { FwdCall k; int first, n; double share; std::string suffix; };
static std::string part_suffix(int first, int n) { return "@" + std::to_string(first) + "+" + std::to_string(n); }
template <typename F>
static int for_each_part(const FwdCall& k, int B, F&& f)
{
    if (!k.split) return f(LaunchPart{k, 0, B, 1.0, ""});
    for (int i = 0; i < 2; ++i) {
        const int first = i ? k.split->n0 : 0, n = i ? B - k.split->n0 : k.split->n0;
        LaunchPart part{k, first, n, (double)n / B, part_suffix(first, n)};
        part.k.split = nullptr;
        if (i) { part.k.stream = k.split->second->stream; part.k.scratch = k.split->second; }
        if (int rc = f(part)) return rc;
    }
    return PMX_OK;
}
// Where image `first` of a launch starts in the buffer `ptr` points into, `per_image` floats an image: first * per_image, except in act0 / act1
// under two chains.  The chains drift apart by layers, and act0 / act1 hold layers of different sizes in turn: at the image offset of each
// layer, a later, smaller layer of one chain would land in what the other chain still reads of an earlier, larger one.  So there the second
// chain starts at a distance that no layer of the first reaches -- n0 images of the largest layer the buffer ever holds (act0: conv1_1's
// output, 64 floats per input pixel; act1: conv1_2's pooled output, 16); every other buffer holds layers of one size only (cat, brA, brB,
// brT at 1/8 resolution; in16) and keeps the image offset.
static size_t image_offset(const FwdCall& k, int first, const float* ptr, size_t per_image)
{
    const NetBufs& ws = k.ws;
    if (k.split && ptr >= ws.act0 && ptr < ws.act0 + ws.act0.capacity()) return (size_t)first * k.split->net_px * 64;
    if (k.split && ptr >= ws.act1 && ptr < ws.act1 + ws.act1.capacity()) return (size_t)first * k.split->net_px * 16;
    return (size_t)first * per_image;
}
// the operands of images [first, first + n) of the launch `io` describes (k: the call of the whole launch)
static ConvIO conv_images(const FwdCall& k, const ConvIO& io, int first, int n)
{
    const size_t pin = (size_t)io.H * io.W * io.lda, pout = (size_t)(io.pool ? io.H / 2 : io.H) * (io.pool ? io.W / 2 : io.W) * io.ldc;
    ConvIO s = io;
    for (int g = 0; g < 2; ++g) {
        if (io.in[g]) s.in[g] += image_offset(k, first, io.in[g], pin);
        if (io.out[g]) s.out[g] += image_offset(k, first, io.out[g], pout);
    }
    s.B = n;
    return s;
}

// The plan of the whole batch, launched once per chain on the chain's images.  Probe: whether a launch of either half is the launch the plan
// describes (the merged tails are a property of the image count) and what the automatic rule says of a 7x7 layer.
static int launch_plan_chains(pmx_ctx* c, const FwdCall& k, const ConvPlan& p)
{
    ChainSplit& s = *k.split;
    const ConvArgs& a = p.a;
    if (s.probe) {
        if (p.form == FORM_WINO_RUN && p.tail_g)
            for (int n : {s.n0, a.B - s.n0}) {
                ConvArgs h = a;
                h.B = n;
                if (wino_tail_merged(c, h) != wino_tail_merged(c, a)) s.ok = false;
            }
        if (p.ks == 7 && !batch_chains_rounds(wino_opts(c, k, p.ks, p.groups, a.lda), p.form == FORM_WINO || p.form == FORM_WINO_RUN, p.form == FORM_WINO_RUN,
                                              p.tail_g, a.cout_pad, s.n0, a.B - s.n0, a.H, a.W)) s.rounds = false;
        return PMX_OK;
    }
    return for_each_part(k, a.B, [&](const LaunchPart& part) {
        ConvPlan q = p;
        args_io(q.a, conv_images(k, p.io, part.first, part.n));
        if (q.prof) { q.pf.flops *= part.share; q.pf.bytes *= part.share; q.pf.issued *= part.share; q.pf.suffix = part.suffix; }
        return launch_plan(c, part.k, q);
    });
}

// one layer of a forward: plan + launch.  A batch whose plain launch would end in a part-filled round of the CUs is cut in two first: the
// images of the whole rounds, then the rest through the selection of THEIR count (conv_select.hip::wino_split_images); each half is an
// ordinary run_conv on its images, whose profile labels end in `half` = "@<first image>+<count>" (null: a whole batch)
static int run_conv(pmx_ctx* c, const FwdCall& k, const char* label, PackedLayer* L0, PackedLayer* L1, const ConvIO& io, const char* half = nullptr)
{
    const bool seg = k.seg && io.level >= 0;
    const int B = io.B, groups = L1 ? 2 : 1;
    int rc;
    if (!seg && !half && c->opt_wino_split && B >= 2 && L0->ks > 1 && c->opt_precision != 2 && wino_layers_ok(L0, L1)) {
        const int n0 = wino_split_images(wino_opts(c, k, L0->ks, groups, io.lda), L0->ks, L0->cin_pad, L0->cout_pad, L0->cout, io.ldc, B, groups, io.H, io.W, io.pool);
        if (n0 > 0 && n0 < B && k.split) {      // (a cut by images is a plan of its own per side: no chains over it)
            PMX_CHECK(k.split->probe, PMX_ERR_STATE, "two chains: layer %s is cut in two by images", label ? label : "?");
            k.split->ok = false;
            return PMX_OK;
        }
        if (n0 > 0 && n0 < B) {
            if ((rc = run_conv(c, k, label, L0, L1, conv_images(k, io, 0, n0), part_suffix(0, n0).c_str()))) return rc;
            return run_conv(c, k, label, L0, L1, conv_images(k, io, n0, B - n0), part_suffix(n0, B - n0).c_str());
        }
    }
    ConvPlan p;
    if ((rc = plan_conv(c, k, p, label, L0, L1, io))) return rc;
    if (half && p.prof) p.pf.suffix = half;
    return k.split ? launch_plan_chains(c, k, p) : launch_plan(c, k, p);
}

// the two 1x1 layers that end a stage (A: 128 -> cmid + ReLU, B: cmid -> cout [+ ReLU]) as ONE launch when the shapes allow
// (else, or with option fuse_pairs = 0, as two run_conv launches through `mid`): bit-identical either way.  A, Bl: the (up to two) groups of
// the two layers; io: A's input and B's output, io.relu = B's ReLU; keep_mid: `mid` must hold the middle activation: two launches
static int run_pair(pmx_ctx* c, const FwdCall& k, const char* labelA, const char* labelB, PackedLayer* const (&A)[2], PackedLayer* const (&Bl)[2],
                    const ConvIO& io, const ConvBuf& mid, bool keep_mid = false)
{
    const PackedLayer& LA = *A[0];
    const PackedLayer& LB = *Bl[0];
    const int groups = A[1] ? 2 : 1;
    // (heterogeneous forward: a 1x1 layer only sees pixels -- the segments' maps are one run of pix[level] pixels)
    const bool seg = k.seg && io.level >= 0;
    const bool ok = !keep_mid && c->opt_fuse_pairs && c->opt_kernel_gen >= 6 && LA.ks == 1 && LB.ks == 1 && LA.cin_pad == 128 && LB.cin == LA.cout &&
                    conv_pair_supported(LA.cin, LA.cout, LB.cout_pad) && (groups == 1 || Bl[1]->cout_pad == LB.cout_pad);
    int rc;
    PMX_CHECK(ok || !seg, PMX_ERR_INVALID, "heterogeneous forward: the 1x1 pair %s + %s has no fused form", labelA, labelB);
    if (!ok) {
        ConvIO a = io, b = io;
        for (int g = 0; g < 2; ++g) a.out[g] = mid.p[g], b.in[g] = mid.p[g];
        a.ldc = b.lda = mid.ld;
        a.relu = 1;
        if ((rc = run_conv(c, k, labelA, A[0], A[1], a))) return rc;
        return run_conv(c, k, labelB, Bl[0], Bl[1], b);
    }
    if (k.split && k.split->probe) return PMX_OK;
    auto pixels = [&](int n) { return seg ? k.seg->pix[io.level] : (long long)n * io.H * io.W; };
    const long long npix = pixels(io.B);
    PairArgs p;
    memset(&p, 0, sizeof p);
    double flops = 0;
    for (int g = 0; g < groups; ++g) {
        p.g[g].w1 = A[g]->d_w; p.g[g].b1 = A[g]->d_b; p.g[g].w2 = Bl[g]->d_w; p.g[g].b2 = Bl[g]->d_b; p.g[g].cout = Bl[g]->cout;
        flops += 2.0 * (double)npix * ((double)A[g]->cout * A[g]->cin + (double)Bl[g]->cout * Bl[g]->cin);
    }
    p.lda = io.lda; p.ldc = io.ldc; p.cmid = LA.cout; p.cout_pad = LB.cout_pad; p.relu2 = io.relu;
    const std::string name = std::string(labelA) + "+" + labelB + "|conv1x1_pair_c" + std::to_string(LA.cout) + "_n" + std::to_string(LB.cout_pad);
    const double bytes = 4.0 * (double)npix * groups * (LA.cin + LB.cout);
    return for_each_part(k, io.B, [&](const LaunchPart& part) {      // (two chains: the launch over each chain's pixels)
        const ConvIO s = conv_images(k, io, part.first, part.n);
        PairArgs q = p;
        q.npix = pixels(part.n);
        for (int g = 0; g < groups; ++g) { q.g[g].in = s.in[g]; q.g[g].out = s.out[g]; }
        int rc;
        if (c->prof_on == 1 && (rc = prof_begin(c, part.k, name + part.suffix, flops * part.share, bytes * part.share))) return rc;
        if ((rc = conv_pair_launch(q, groups, part.k.stream))) return rc;
        return prof_end(c, part.k);
    });
}

// conv1_1 + conv1_2 have the shapes conv1_wino_kernel is written for (3 -> 64 -> 64, fp32)?
static bool conv1_pairable(const pmx_ctx* c)
{
    const PackedLayer& L1 = c->layers[c->index.at("conv1_1")];
    const PackedLayer& L2 = c->layers[c->index.at("conv1_2")];
    return c->opt_precision == 0 && c->opt_force[3] < 0 && L1.cin == 3 && L1.cout == 64 && L2.cin == 64 && L2.cout == 64;
}
// a forward that retains the trunk (pmx_backward_enable(ctx, 2); the conditions of pmx_forward_from_in16's `keep`): conv1_1 and conv1_2 run
// as two launches that store both outputs, so neither fused form applies and a uint8 input is preprocessed into in16 first
static bool trunk_retaining(const pmx_ctx* c, const FwdCall& k)
{
    return c->bw.on == 2 && c->kind == NET_POSE && c->ls_on && c->lg_on && c->opt_precision == 0 && !k.seg;
}
// which form conv1_1 -> conv1_2 (+ pool) takes: *fuse: one launch (direct conv1_2 on 8 x 16 x 64 tiles: large maps); returns true for
// conv1_2 as Winograd F(2x2, 3x3) on 16 x 16 squares (conv1_wino.hip): wherever the Winograd kernels are allowed (conv_algo >= 1) and the
// launch has at least one block per CU (smaller launches: the 8 x 16 direct tiles give twice the blocks); conv1_wino = 2: always
static bool conv1_form(const pmx_ctx* c, const FwdCall& k, int B, int H, int W, bool* fuse_out)
{
    if (trunk_retaining(c, k)) {
        if (fuse_out) *fuse_out = false;
        return false;
    }
    const PackedLayer& L2 = c->layers[c->index.at("conv1_2")];
    const int v2 = conv_pick_variant(3, L2.cout_pad, H, W, B, c->opt_force[3], c->opt_kernel_gen, 1, L2.cin, 0, c->num_cus);
    const bool fuse = c->opt_fuse_conv1 && c->opt_kernel_gen >= 6 && conv1_pairable(c) && !strcmp(conv_variant(v2).name, "conv3x3_v5_t8x16_n64");
    const bool pair_ok = conv1_pairable(c) && H % 2 == 0 && W % 2 == 0;
    if (fuse_out) *fuse_out = fuse;
    return pair_ok && c->opt_conv1_wino && k.conv_algo >= 1 &&
           (c->opt_conv1_wino == 2 || (fuse && (long long)B * ((H + 15) / 16) * ((W + 15) / 16) >= c->num_cus));
}

static int run_conv1(pmx_ctx* c, const FwdCall& k, int B, int H, int W)
{
    NetBufs& ws = k.ws;
    PackedLayer& L1 = c->layers[c->index.at("conv1_1")];
    PackedLayer& L2 = c->layers[c->index.at("conv1_2")];
    bool fuse = false;
    const bool seg = k.seg != nullptr;
    const bool wino1 = seg ? conv1_pairable(c) : conv1_form(c, k, B, H, W, &fuse);
    const uint8_t* const in_u8 = k.in_u8;
    PMX_CHECK(!in_u8 || wino1, PMX_ERR_STATE, "conv1: a uint8 input without the kernel that preprocesses it");
    int rc;
    // f16 mode, heterogeneous: pmx_forward_from_u8 has preprocessed the segments' pixels into in16; both layers on the level-0 rectangle tables
    const bool f16_seg = seg && c->opt_precision == 2;
    PMX_CHECK(!f16_seg || !in_u8, PMX_ERR_STATE, "conv1: a uint8 input in f16 mode");
    PMX_CHECK(!seg || f16_seg || (wino1 && in_u8), PMX_ERR_INVALID, "heterogeneous forward: needs conv1 as conv1_wino_kernel on a uint8 input");
    const ConvBuf in16 = ConvBuf::one(ws.in16, PMX_IN_C), act0 = ConvBuf::one(ws.act0, 64), act1 = ConvBuf::one(ws.act1, 64);
    if (f16_seg || (!fuse && !wino1)) {
        if ((rc = run_conv(c, k, "conv1_1", &L1, nullptr, conv_io(in16, act0, B, H, W, 1, 0, 0)))) return rc;
        return run_conv(c, k, "conv1_2", &L2, nullptr, conv_io(act0, act1, B, H, W, 1, 1, 0));
    }
    if (k.split && k.split->probe) return PMX_OK;
    // one launch: group 0 is conv1_2 (in16 -> pooled act1), group 1 carries conv1_1's weights and, for the kernel that preprocesses the
    // uint8 batch itself (pmx_forward_from_u8), the pixels and their divisor
    const ConvIO io = conv_io(in16, act1, B, H, W, 1, 1);
    ConvArgs a;
    memset(&a, 0, sizeof a);
    args_io(a, io);
    a.g[0].w = L2.d_w; a.g[0].bias = L2.d_b; a.g[0].cout = L2.cout; a.g[1].w = L1.d_w; a.g[1].bias = L1.d_b;
    a.nch = L2.nch; a.cout_pad = L2.cout_pad;
    if (wino1) {
        if ((rc = ensure_wino_pack(k.stream, L2)) || (rc = ensure_conv1_pack(k.stream, L1))) return rc;
        a.g[0].w = L2.d_ww; a.g[1].w = L1.d_ww;
        if (in_u8) a.kbounds = (unsigned long long)__builtin_bit_cast(unsigned, k.in_div);
        if (seg) { a.nseg = (int)k.seg->segs.size(); a.segs = k.seg->table(PMX_SEG_CONV1); a.seg_tiles = k.seg->tiles[PMX_SEG_CONV1]; }
    }
    // the profile entry, per input pixel (whole numbers, so a part's figures are exact whichever way they are multiplied out)
    const double f1 = 2.0 * 9.0 * (double)L1.cout * L1.cin, f2 = 2.0 * 9.0 * (double)L2.cout * L2.cin;
    const ConvProf pf = wino1 ? ConvProf{"conv1_1+conv1_2|conv_wino1_f2x2_t16x16", f1 + f2, (in_u8 ? 3.0 : 4.0 * 3) + 4.0 * (64 / 4), f1 + f2 * 16.0 / 36.0, ""}
                              : ConvProf{"conv1_1+conv1_2|conv1_fused_t8x16_n64", f1 + f2, 4.0 * (3 + 64 / 4), f1 + f2, ""};
    return for_each_part(k, B, [&](const LaunchPart& part) {      // (two chains: the form of the whole batch over each chain's images)
        ConvArgs q = a;
        args_io(q, conv_images(k, io, part.first, part.n));
        if (wino1 && in_u8) q.g[1].in = reinterpret_cast<const float*>(in_u8 + (size_t)part.first * H * W * 3);
        int rc;
        if (c->prof_on == 1) {
            const double np = seg ? (double)k.seg->pix[0] : (double)part.n * H * W;
            if ((rc = prof_begin(c, part.k, pf.name + part.suffix, np * pf.flops, np * pf.bytes, np * pf.issued))) return rc;
        }
        if ((rc = wino1 ? conv1_wino_launch(q, part.k.stream) : conv1_fused_launch(q, part.k.stream))) return rc;
        return prof_end(c, part.k);
    });
}

// conv1_1 ... conv4_2, the VGG stem all three networks share (CocoPoseNet.py:136-149, FaceNet.py:78-92): act1 and act0 in turn, the three
// F.max_pooling_2d fused into conv1_2, conv2_2, conv3_4; the result (1/8 resolution, 512 channels) in act1
// (level = the resolution level of the layer's input, read only by a heterogeneous forward: pmx_multi.hip)
// (last_out: where conv4_2 writes instead -- a retaining forward, pmx_backward_enable)
static int run_stem(pmx_ctx* c, const FwdCall& k, int B, int H, int W, float* last_out = nullptr)
{
    static const struct { const char* name; int cin, cout, level, pool; } stem[] = {
        {"conv2_1", 64, 128, 1, 0}, {"conv2_2", 128, 128, 1, 1}, {"conv3_1", 128, 256, 2, 0}, {"conv3_2", 256, 256, 2, 0},
        {"conv3_3", 256, 256, 2, 0}, {"conv3_4", 256, 256, 2, 1}, {"conv4_1", 256, 512, 3, 0}, {"conv4_2", 512, 512, 3, 0}};
    int rc = run_conv1(c, k, B, H, W);
    float* in = k.ws.act1;
    float* out = k.ws.act0;
    for (const auto& s : stem) {
        if (rc) break;
        if (last_out && &s == &stem[7]) out = last_out;
        rc = run_conv(c, k, s.name, &c->layers[c->index.at(s.name)], nullptr,
                      conv_io(ConvBuf::one(in, s.cin), ConvBuf::one(out, s.cout), B, H >> s.level, W >> s.level, 1, s.pool, s.level));
        std::swap(in, out);
    }
    return rc;
}

// The stem of a forward that retains the trunk (BwState in pmx_ctx.h; include/pose_mi355x.h: pmx_backward_enable, mode 2): every layer
// writes its post-ReLU output into its slot of the trunk store with its own launch, the three pooling layers un-pooled, and
// maxpool_nhwc_kernel writes the pooled map the next layer reads.  conv4_2 writes x42, as in mode 1.
static int run_stem_retaining(pmx_ctx* c, const FwdCall& k, int B, int H, int W, float* x42)
{
    BwState& bw = c->bw;
    PMX_CHECK(!k.in_u8, PMX_ERR_STATE, "retaining stem: a uint8 input that no kernel preprocesses");
    PMX_CHECK((size_t)B * H * W <= bw.cap_px * 64, PMX_ERR_CAPACITY, "forward: %d x %d x %d input pixels, the trunk store holds %zu", B, H, W, bw.cap_px * 64);
    float* in = k.ws.in16;
    int lda = PMX_IN_C, pools = 0, rc;
    for (int t = 0; t < PMX_TRUNK_LAYERS; ++t) {
        const TrunkDesc& d = pmx_trunk_desc[t];
        const int h = H >> d.level, w = W >> d.level;
        float* out = t == PMX_TRUNK_LAYERS - 1 ? x42 : bw.t_act + bw.t_a_off[t];
        if ((rc = run_conv(c, k, d.name, &c->layers[bw.t_layer[t]], nullptr, conv_io(ConvBuf::one(in, lda), ConvBuf::one(out, d.cout), B, h, w, 1, 0, d.level)))) return rc;
        in = out; lda = d.cout;
        if (!d.pool) continue;
        float* pooled = bw.t_act + bw.t_p_off[pools++];
        if (c->prof_on == 1) {
            const std::string label = std::string("pool:") + d.name + "|maxpool_nhwc";
            if ((rc = prof_begin(c, k, label, 0, 4.0 * B * h * w * d.cout * 1.25))) return rc;
        }
        if ((rc = maxpool_nhwc_launch(out, d.cout, pooled, d.cout, B, h, w, d.cout, k.stream))) return rc;
        if ((rc = prof_end(c, k))) return rc;
        in = pooled;
    }
    return PMX_OK;
}

// FaceNet / HandNet forward (models/FaceNet.py:78-160): one branch, groups = 1 everywhere
static int forward_cpm(pmx_ctx* c, const FwdCall& k, int B, int H, int W)
{
    NetBufs& ws = k.ws;
    auto L = [&](const char* n) { return &c->layers[c->index.at(n)]; };
    int rc;
    const int H8 = H / 8, W8 = W / 8;
    const int CC = c->cat_c;
    // the buffers of the graph: cat = [128 feature channels | the stage's heat maps]
    const ConvBuf act0 = ConvBuf::one(ws.act0, 512), act1 = ConvBuf::one(ws.act1, 512), cat = ConvBuf::one(ws.cat, CC), heat = ConvBuf::one(ws.cat + c->cat_heat, CC);
    const ConvBuf brA = ConvBuf::one(ws.brA, 128), brB = ConvBuf::one(ws.brB, 128), brT = ConvBuf::one(ws.brT, 512);
    auto conv = [&](const char* name, const ConvBuf& in, const ConvBuf& out) { return run_conv(c, k, name, L(name), nullptr, conv_io(in, out, B, H8, W8, 1, 0)); };
    auto pair = [&](const char* nameA, const char* nameB, const ConvBuf& in, const ConvBuf& mid) {
        return run_pair(c, k, nameA, nameB, {L(nameA), nullptr}, {L(nameB), nullptr}, conv_io(in, heat, B, H8, W8, 0, 0), mid);
    };
    if ((rc = run_stem(c, k, B, H, W)) || (rc = conv("conv4_3", act1, act0)) || (rc = conv("conv4_4", act0, act1)) || (rc = conv("conv5_1", act1, act0)) ||
        (rc = conv("conv5_2", act0, act1)) || (rc = conv("conv5_3_CPM", act1, cat))) return rc;               // feature_map -> cat[:, 0:128]
    // conv6_1_CPM (reads the 128 feature channels) -> conv6_2_CPM (stage-1 heat maps -> cat[:, 128:128+C])
    if ((rc = pair("conv6_1_CPM", "conv6_2_CPM", cat, brT))) return rc;
    char nm[48], nm2[48];
    for (int s = 2; s <= 6 && s <= c->opt_stop_stage; ++s) {
        for (int i = 1; i <= 5; ++i) {
            snprintf(nm, sizeof nm, "Mconv%d_stage%d", i, s);
            if ((rc = conv(nm, i == 1 ? cat : i % 2 == 0 ? brA : brB, i % 2 == 1 ? brA : brB))) return rc;
        }
        snprintf(nm, sizeof nm, "Mconv6_stage%d", s);
        snprintf(nm2, sizeof nm2, "Mconv7_stage%d", s);
        if ((rc = pair(nm, nm2, brA, brB))) return rc;
    }
    c->maps_valid = true; c->maps_external = false;
    c->cur_B = B; c->cur_fh = H8; c->cur_fw = W8;
    c->cur_segs.clear();
    c->pp_valid = false;
    return PMX_OK;
}

int pmx_forward_from_in16(pmx_ctx* c, const FwdCall& k, int B, int H, int W)
{
    PMX_CHECK(!k.seg || c->kind == NET_POSE, PMX_ERR_INVALID, "heterogeneous forward: posenet only");
    if (c->kind != NET_POSE) return forward_cpm(c, k, B, H, W);
    NetBufs& ws = k.ws;
    auto L = [&](const char* n) { return &c->layers[c->index.at(n)]; };
    int rc;
    const int H8 = H / 8, W8 = W / 8;
    // validation-loss hook (pmx_loss.hip; uniform batches): the stage's outputs lie in the cat slices until the next stage's last launch
    const bool hook = c->ls_on && !k.seg;
    // (the hook and the retention read the context's own cat slices on the context's stream)
    PMX_CHECK(!hook || (&ws == static_cast<NetBufs*>(c) && k.stream == c->stream), PMX_ERR_STATE, "forward: the validation-loss hook covers the context's own working set only");
    // retention (pmx_backward_enable; include/pose_mi355x.h): every layer writes where the backward will read it -- the slots of c->bw.act
    // instead of act1 / act0 / brA / brB / brT (same leading dimensions: same plans, same bits), the 1x1 pairs unfused
    BwState& bw = c->bw;
    const bool keep = bw.on && hook && c->lg_on && c->opt_precision == 0;
    PMX_CHECK(!k.split || !hook, PMX_ERR_STATE, "forward: two chains under the validation-loss hook");
    bw.valid = bw.done = bw.trunk_done = false;
    const long long npix8 = (long long)B * H8 * W8;
    PMX_CHECK(!keep || (size_t)npix8 <= bw.cap_px, PMX_ERR_CAPACITY, "forward: %lld map pixels, the backward store holds %zu", npix8, bw.cap_px);
    auto slot = [&](int sl, float* else_) { return keep ? bw.act + bw.slot[sl].a_off : else_; };
    float* const x42 = slot(PMX_BW_X42, ws.act1);
    float* const a43 = slot(PMX_BW_C43, ws.act0);
    auto keep_stage = [&](int sl) {      // the stage's 57 (64) channels of cat -> the store
        return keep ? bwd_copy_cols_launch(ws.cat + PMX_CAT_PAF, PMX_CAT_C, bw.act + bw.slot[sl].a_off, 64, npix8, 64, k.stream) : PMX_OK;
    };
    // stem (CocoPoseNet.py:136-151)
    if ((rc = keep && bw.on == 2 ? run_stem_retaining(c, k, B, H, W, x42) : run_stem(c, k, B, H, W, keep ? x42 : nullptr))) return rc;
    // Everything below runs at 1/8 resolution (level 3: read only by a heterogeneous forward, pmx_multi.hip).  L1 = PAF branch, L2 = heat-map
    // branch, the two groups of one launch: side by side in every buffer (br), both reading the whole concat buffer (cat_in), writing its
    // PAF and heat-map slices (maps)
    auto br = [](float* p, int ch = 128) { return ConvBuf::two(p, ch, 2 * ch); };
    const ConvBuf cat_in = ConvBuf::two(ws.cat, 0, PMX_CAT_C), maps = ConvBuf::two(ws.cat + PMX_CAT_PAF, PMX_CAT_HEAT - PMX_CAT_PAF, PMX_CAT_C);
    auto conv = [&](const char* label, PackedLayer* L0, PackedLayer* L1, const ConvBuf& in, const ConvBuf& out) {
        return run_conv(c, k, label, L0, L1, conv_io(in, out, B, H8, W8, 1, 0, 3));
    };
    if ((rc = conv("conv4_3_CPM", L("conv4_3_CPM"), nullptr, ConvBuf::one(x42, 512), ConvBuf::one(a43, 256)))) return rc;
    if ((rc = conv("conv4_4_CPM", L("conv4_4_CPM"), nullptr, ConvBuf::one(a43, 256), ConvBuf::one(ws.cat + PMX_CAT_FEAT, PMX_CAT_C)))) return rc;
    // stage 1 (CocoPoseNet.py:154-165)
    float* const s51 = slot(PMX_BW_S1 + 0, ws.brA);
    float* const s52 = slot(PMX_BW_S1 + 1, ws.brB);
    float* const s53 = slot(PMX_BW_S1 + 2, ws.brA);
    float* const s54 = slot(PMX_BW_S1 + 3, ws.brT);
    if ((rc = conv("conv5_1_CPM", L("conv5_1_CPM_L1"), L("conv5_1_CPM_L2"), cat_in, br(s51)))) return rc;
    if ((rc = conv("conv5_2_CPM", L("conv5_2_CPM_L1"), L("conv5_2_CPM_L2"), br(s51), br(s52)))) return rc;
    if ((rc = conv("conv5_3_CPM", L("conv5_3_CPM_L1"), L("conv5_3_CPM_L2"), br(s52), br(s53)))) return rc;
    // conv5_4 (128 -> 512, ReLU) -> conv5_5 (512 -> 38 | 19): one launch
    if ((rc = run_pair(c, k, "conv5_4_CPM", "conv5_5_CPM", {L("conv5_4_CPM_L1"), L("conv5_4_CPM_L2")}, {L("conv5_5_CPM_L1"), L("conv5_5_CPM_L2")},
                       conv_io(br(s53), maps, B, H8, W8, 0, 0, 3), br(s54, 512), keep))) return rc;
    int n_stages = 1;
    if (hook && (rc = pmx_loss_stage(c, 1, B, H8, W8))) return rc;
    if ((rc = keep_stage(PMX_BW_S1 + 4))) return rc;
    // stages 2-6 (CocoPoseNet.py:168-260)
    char n1[48], n2[48], m1[48], m2[48], lab[48], lab2[48];
    for (int s = 2; s <= 6 && s <= c->opt_stop_stage; ++s) {
        ConvBuf in = cat_in;
        for (int i = 1; i <= 5; ++i) {
            snprintf(n1, sizeof n1, "Mconv%d_stage%d_L1", i, s);
            snprintf(n2, sizeof n2, "Mconv%d_stage%d_L2", i, s);
            snprintf(lab, sizeof lab, "Mconv%d_stage%d", i, s);
            const ConvBuf o = br(slot(PMX_BW_M(s, i), i % 2 == 1 ? ws.brA : ws.brB));
            if ((rc = conv(lab, L(n1), L(n2), in, o))) return rc;
            in = o;
        }
        // Mconv6 (1x1 128 -> 128, ReLU; reads Mconv5's output in brA) -> Mconv7 (1x1 128 -> 38 | 19, into the cat slices): one launch
        snprintf(n1, sizeof n1, "Mconv6_stage%d_L1", s); snprintf(n2, sizeof n2, "Mconv6_stage%d_L2", s);
        snprintf(m1, sizeof m1, "Mconv7_stage%d_L1", s); snprintf(m2, sizeof m2, "Mconv7_stage%d_L2", s);
        snprintf(lab, sizeof lab, "Mconv6_stage%d", s); snprintf(lab2, sizeof lab2, "Mconv7_stage%d", s);
        if ((rc = run_pair(c, k, lab, lab2, {L(n1), L(n2)}, {L(m1), L(m2)}, conv_io(in, maps, B, H8, W8, 0, 0, 3), br(slot(PMX_BW_M(s, 6), ws.brB)), keep))) return rc;
        n_stages = s;
        if (hook && (rc = pmx_loss_stage(c, s, B, H8, W8))) return rc;
        if ((rc = keep_stage(PMX_BW_M(s, 7)))) return rc;
    }
    if (hook && (rc = pmx_loss_finish(c, n_stages, B, H8, W8))) return rc;
    if (keep) { bw.valid = true; bw.stages = n_stages; bw.B = B; bw.fh = H8; bw.fw = W8; bw.t_H = H; bw.t_W = W; }
    if (k.split && k.split->probe) return PMX_OK;      // (nothing ran)
    c->maps_valid = true; c->maps_external = false;
    c->cur_B = B; c->cur_fh = H8; c->cur_fw = W8;
    c->cur_segs.clear();             // (a heterogeneous forward: forward_segments installs the layout of its tables)
    c->pp_valid = false;
    return PMX_OK;
}

int pmx_check_weights(pmx_ctx* c)
{
    int missing = 0;
    for (auto& l : c->layers) missing += l.set ? 0 : 1;
    PMX_CHECK(missing == 0, PMX_ERR_WEIGHTS, "forward: %d of %d layers have no weights", missing, (int)c->layers.size());
    return PMX_OK;
}
static int check_forward_args(pmx_ctx* c, const void* p, int B, int H, int W)
{
    PMX_CHECK(c && p, PMX_ERR_INVALID, "forward: null arg");
    PMX_CHECK(B >= 1 && B <= c->max_batch, PMX_ERR_CAPACITY, "forward: batch %d outside 1..%d", B, c->max_batch);
    PMX_CHECK(H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0, PMX_ERR_INVALID, "forward: H, W must be multiples of 8 (got %d x %d)", H, W);
    PMX_CHECK((size_t)H * W <= (size_t)c->max_h * c->max_w, PMX_ERR_CAPACITY, "forward: %d x %d exceeds the context capacity %d x %d",
              H, W, c->max_h, c->max_w);
    if (int rc = pmx_check_weights(c)) return rc;
    return c->ls_on ? pmx_loss_check(c, B, H, W) : PMX_OK;
}

extern "C" int pmx_forward_u8(pmx_ctx* c, const uint8_t* img, int B, int H, int W, int on_device)
{
    int rc = check_forward_args(c, img, B, H, W);
    if (rc) return rc;
    PMX_DEV(c);
    const uint8_t* d = img;
    if (!on_device) {
        PMX_HIP(hipMemcpyAsync(c->u8_tmp, img, (size_t)B * H * W * 3, hipMemcpyHostToDevice, c->stream));
        d = c->u8_tmp;
    }
    return pmx_forward_from_u8(c, pmx_call(c), d, B, H, W, c->kind == NET_POSE ? 255.0f : 256.0f);
}

int pmx_forward_from_u8(pmx_ctx* c, const FwdCall& k, const uint8_t* d, int B, int H, int W, float divisor)
{
    int rc;
    if (k.seg && c->opt_precision == 2) {
        // f16 mode, heterogeneous forward: the segments' uint8 pixels lie end to end in `d` (forward_segments), so the preprocessing is one
        // per-pixel pass over the flat run of pix[0] pixels; conv1_1 then reads in16 through the level-0 rectangle table
        const long long np0 = k.seg->pix[0];
        PMX_CHECK(np0 >= 1 && np0 <= (long long)c->max_batch * c->max_h * c->max_w && np0 < (1ll << 31), PMX_ERR_CAPACITY,
                  "heterogeneous forward: %lld input pixels", np0);
        if (c->prof_on == 1 && (rc = prof_begin(c, k, "prep_u8|prep_u8", 0, (double)np0 * (3 + 64)))) return rc;
        if ((rc = launch_prep_u8(d, k.ws.in16, 1, 1, (int)np0, divisor, k.stream))) return rc;
        if ((rc = prof_end(c, k))) return rc;
        return pmx_forward_from_in16(c, k, B, H, W);
    }
    if (k.seg || conv1_form(c, k, B, H, W, nullptr)) {                        // conv1_wino_kernel reads the uint8 pixels and preprocesses them in its patch load
        FwdCall ku = k;
        ku.in_u8 = d; ku.in_div = divisor;
        return pmx_forward_from_in16(c, ku, B, H, W);
    }
    auto prep = [&](const LaunchPart& part) {      // (two chains: each preprocesses its own images)
        const size_t px0 = (size_t)part.first * H * W;
        int rc;
        if (c->prof_on == 1 && (rc = prof_begin(c, part.k, "prep_u8|prep_u8" + part.suffix, 0, (double)part.n * H * W * (3 + 64)))) return rc;
        if ((rc = launch_prep_u8(d + px0 * 3, k.ws.in16 + px0 * PMX_IN_C, part.n, H, W, divisor, part.k.stream))) return rc;
        return prof_end(c, part.k);
    };
    if (!(k.split && k.split->probe) && (rc = for_each_part(k, B, prep))) return rc;
    return pmx_forward_from_in16(c, k, B, H, W);
}

extern "C" int pmx_forward_f32(pmx_ctx* c, const float* x, int B, int H, int W, int on_device)
{
    int rc = check_forward_args(c, x, B, H, W);
    if (rc) return rc;
    PMX_DEV(c);
    const float* d = x;
    if (!on_device) {
        PMX_HIP(hipMemcpyAsync(c->nchw_tmp, x, (size_t)B * H * W * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        d = c->nchw_tmp;
    }
    if ((rc = launch_prep_f32(d, c->in16, B, H, W, c->stream))) return rc;
    return pmx_forward_from_in16(c, pmx_call(c), B, H, W);
}

// OpenCV INTER_LINEAR uint8 tables for one axis: [idx0 | idx1 | coef0 | coef1], each `dst` ints.
// fx = float((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double; s = floor(fx); fx -= s;
// s < 0 -> (0, fx = 0); s >= src - 1 -> (src - 1, fx = 0); coefficients cvRound((1 - fx) * 2048), cvRound(fx * 2048).
void pmx_make_resize_table(int dst, int src, int* tab)
{
    const double scale = 1.0 / ((double)dst / (double)src);
    for (int d = 0; d < dst; ++d) {
        float f = (float)(((double)d + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f = f - (float)s;
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= src - 1) { s = src - 1; f = 0.f; }
        tab[d] = s;
        tab[dst + d] = s + 1 < src - 1 ? s + 1 : src - 1;
        tab[2 * dst + d] = (int)lrintf((1.0f - f) * 2048.0f);
        tab[3 * dst + d] = (int)lrintf(f * 2048.0f);
    }
}

// uint8 images of one original size -> cv2.resize(..., (w, h)) on the device -> network forward
extern "C" int pmx_forward_u8_resized(pmx_ctx* c, const uint8_t* img, int B, int src_h, int src_w, int h, int w, int on_device)
{
    if (src_h == h && src_w == w) return pmx_forward_u8(c, img, B, h, w, on_device);     // identity (pose_detector.py:493)
    int rc = check_forward_args(c, img, B, h, w);
    if (rc && rc != PMX_ERR_WEIGHTS) return rc;      // without weights the resize still runs (pmx_get_resized), then
                                                     // pmx_forward_u8 below reports PMX_ERR_WEIGHTS
    PMX_CHECK(src_h >= 1 && src_w >= 1, PMX_ERR_INVALID, "forward_u8_resized: bad source size");
    PMX_DEV(c);
    const size_t nsrc = (size_t)B * src_h * src_w * 3;
    const uint8_t* d = img;
    if (!on_device) {
        if ((rc = c->u8_src.ensure(nsrc, c->stream))) return rc;
        PMX_HIP(hipMemcpyAsync(c->u8_src, img, nsrc, hipMemcpyHostToDevice, c->stream));
        d = c->u8_src;
    }
    const size_t ntab = (size_t)4 * (w + h);
    if ((rc = c->rs_tab.ensure(ntab, c->stream))) return rc;
    std::vector<int> tab(ntab);
    pmx_make_resize_table(w, src_w, tab.data());
    pmx_make_resize_table(h, src_h, tab.data() + 4 * w);
    const int key[4] = {src_h, src_w, h, w};
    if (memcmp(key, c->rs_key, sizeof key)) {      // a call with the sizes of the last one finds its tables on the device and only enqueues
        c->rs_key[0] = 0;                          // (until the upload below is complete)
        PMX_HIP(hipStreamSynchronize(c->stream));     // the table buffer may still be in use by a queued resize
        PMX_HIP(hipMemcpy(c->rs_tab, tab.data(), ntab * sizeof(int), hipMemcpyHostToDevice));
        memcpy(c->rs_key, key, sizeof key);
    }
    if ((rc = pmx_prof_begin(c, "resize_u8|resize_linear_u8", (double)nsrc + (double)B * h * w * 3))) return rc;
    if ((rc = launch_resize_linear_u8(d, c->u8_tmp, c->rs_tab, c->rs_tab + 4 * w, B, src_h, src_w, h, w, c->stream))) return rc;
    if ((rc = pmx_prof_end(c))) return rc;
    return pmx_forward_u8(c, c->u8_tmp, B, h, w, 1);
}

// test / parity accessor: the resized uint8 batch of the last pmx_forward_u8_resized (B x h x w x 3)
extern "C" int pmx_get_resized(pmx_ctx* c, uint8_t* out, int B, int h, int w)
{
    PMX_CHECK(c && out, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(B >= 1 && B <= c->max_batch && (size_t)h * w <= (size_t)c->max_h * c->max_w, PMX_ERR_CAPACITY, "pmx_get_resized: size");
    PMX_DEV(c);
    PMX_HIP(hipMemcpyAsync(out, c->u8_tmp, (size_t)B * h * w * 3, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_get_maps(pmx_ctx* c, float* paf, float* heat)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->maps_valid, PMX_ERR_STATE, "pmx_get_maps: no forward / set_maps yet");
    PMX_CHECK(c->cur_segs.empty(), PMX_ERR_STATE, "pmx_get_maps: the current maps are those of a mixed-size batch (use pmx_get_image_maps)");
    PMX_DEV(c);
    const int B = c->cur_B, fh = c->cur_fh, fw = c->cur_fw;
    PMX_CHECK(c->kind == NET_POSE || !paf, PMX_ERR_INVALID, "pmx_get_maps: facenet / handnet have no PAF output (pass NULL)");
    const size_t np = c->kind == NET_POSE ? (size_t)B * PMX_N_PAF * fh * fw : 0, nh = (size_t)B * c->n_heat * fh * fw;
    if (c->maps_external) {
        if (paf) PMX_HIP(hipMemcpyAsync(paf, c->ext_paf, np * 4, hipMemcpyDeviceToHost, c->stream));
        if (heat) PMX_HIP(hipMemcpyAsync(heat, c->ext_heat, nh * 4, hipMemcpyDeviceToHost, c->stream));
    } else {
        int rc;
        if (paf) {
            if ((rc = launch_nhwc_to_nchw(c->cat, c->nchw_tmp, B, PMX_N_PAF, fh, fw, PMX_CAT_C, PMX_CAT_PAF, c->stream))) return rc;
            PMX_HIP(hipMemcpyAsync(paf, c->nchw_tmp, np * 4, hipMemcpyDeviceToHost, c->stream));
        }
        if (heat) {
            float* tmp = c->nchw_tmp + np;
            if ((rc = launch_nhwc_to_nchw(c->cat, tmp, B, c->n_heat, fh, fw, c->cat_c, c->cat_heat, c->stream))) return rc;
            PMX_HIP(hipMemcpyAsync(heat, tmp, nh * 4, hipMemcpyDeviceToHost, c->stream));
        }
    }
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_set_maps(pmx_ctx* c, const float* paf, const float* heat, int B, int fh, int fw)
{
    PMX_CHECK(c && heat && (paf || c->kind != NET_POSE), PMX_ERR_INVALID, "pmx_set_maps: null arg");
    PMX_CHECK(B >= 1 && B <= c->max_batch, PMX_ERR_CAPACITY, "pmx_set_maps: batch %d outside 1..%d", B, c->max_batch);
    PMX_CHECK(fh >= 1 && fw >= 1, PMX_ERR_INVALID, "pmx_set_maps: bad size");
    PMX_DEV(c);
    const size_t need = (size_t)B * fh * fw;
    int rc;
    if ((rc = c->ext_paf.ensure(need * PMX_N_PAF, c->stream)) || (rc = c->ext_heat.ensure(need * c->n_heat, c->stream))) return rc;
    if (paf) PMX_HIP(hipMemcpyAsync(c->ext_paf, paf, need * PMX_N_PAF * 4, hipMemcpyHostToDevice, c->stream));
    PMX_HIP(hipMemcpyAsync(c->ext_heat, heat, need * c->n_heat * 4, hipMemcpyHostToDevice, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));    // host buffers may be released by the caller
    c->maps_valid = true; c->maps_external = true;
    c->cur_B = B; c->cur_fh = fh; c->cur_fw = fw;
    c->cur_segs.clear();
    c->pp_valid = false;
    return PMX_OK;
}

// ------------------------------------------------------------------------------------- post-process
extern "C" int pmx_set_gaussian(pmx_ctx* c, const double* taps, int radius)
{
    PMX_CHECK(c && taps, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(radius >= 0 && radius <= PMX_GAUSS_MAX_RADIUS, PMX_ERR_INVALID, "pmx_set_gaussian: radius %d > %d", radius, PMX_GAUSS_MAX_RADIUS);
    c->gauss.assign(taps, taps + 2 * radius + 1);
    c->tab_in_h = -1;   // force table rebuild / upload
    if (!c->tab_cache.empty()) {      // the per-size table sets of mixed batches carry the old taps (a setup call: synchronising is fine)
        PMX_DEV(c);
        PMX_HIP(hipDeviceSynchronize());
        c->tab_cache.clear();
    }
    return PMX_OK;
}

void pmx_pp_gauss(const pmx_ctx* c, void* host, void* dev, PPTables& t)
{
    if (c->opt_gpu_branch_peaks) {
        // create_gaussian_kernel(sigma, ksize = 17) (pose_detector.py:38-44): 1/(2 pi sigma^2) exp(-d^2 / 2 sigma^2), NOT
        // normalised to sum 1, applied as a 17x17 zero-padded convolution (:112-113); separable factor per axis
        const int r = 8;
        double g[2 * r + 1];
        const double s2 = PMX_GAUSS_SIGMA * PMX_GAUSS_SIGMA;
        for (int i = -r; i <= r; ++i) g[i + r] = sqrt(1.0 / (s2 * 2.0 * M_PI)) * exp(-0.5 * (double)(i * i) / s2);
        pp_taps_build(g, 2 * r + 1, 1, 1, host, dev, t);
    } else {
        pp_taps_build(c->gauss.data(), (int)c->gauss.size(), 0, 0, host, dev, t);
    }
}

int pmx_ensure_smoothed(pmx_ctx* c, size_t floats)
{
    const int rc = c->smoothed.ensure(floats, c->stream);
    c->pp.smoothed = c->smoothed;       // (null after a failed growth)
    return rc;
}

// The table set of the context for one (network map, up-sampled map) size pair: [grid | taps] (pp_tables.h), built on the host, one upload.
// A failure anywhere in here (the one allocation of a larger set, the upload) leaves the context consistent: c->tab points into what
// c->tab_store holds, or nowhere, and tab_in_h stays invalid, so the next call builds the set again
int pmx_ensure_tables(pmx_ctx* c, int in_h, int in_w, int out_h, int out_w, int flip_x)
{
    if (c->tab_in_h == in_h && c->tab_in_w == in_w && c->tab_out_h == out_h && c->tab_out_w == out_w && c->tab_flip == flip_x) return PMX_OK;
    const size_t grid = pp_grid_bytes(out_h, out_w), bytes = grid + pp_taps_bytes();
    c->tab_in_h = -1;       // until the upload below is complete
    if (int rc = c->tab_store.ensure(bytes, c->stream)) {
        if (!c->tab_store) c->tab = PPTables{};      // (the old set went before the new allocation failed)
        return rc;
    }
    std::vector<double> host(bytes / sizeof(double));
    pp_grid_build(in_h, in_w, out_h, out_w, flip_x, host.data(), c->tab_store.get(), c->tab);
    pmx_pp_gauss(c, host.data() + grid / sizeof(double), c->tab_store + grid, c->tab);
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(c->tab_store, host.data(), bytes, hipMemcpyHostToDevice));
    c->tab_in_h = in_h; c->tab_in_w = in_w; c->tab_out_h = out_h; c->tab_out_w = out_w; c->tab_flip = flip_x;
    return PMX_OK;
}

PPMaps pmx_current_maps(const pmx_ctx* c)
{
    const long long fhw = (long long)c->cur_fh * c->cur_fw;
    const bool paf = c->kind == NET_POSE;
    PPMaps m;
    if (c->maps_external) {          // NCHW copies installed by pmx_set_maps
        m.heat = c->ext_heat; m.paf = paf ? c->ext_paf.get() : nullptr;
        m.sx = 1; m.sy = c->cur_fw; m.sc = fhw;
        m.sbh = c->n_heat * fhw; m.sbp = paf ? PMX_N_PAF * fhw : 0;
    } else {                         // channel slices of the NHWC cat buffer written by the last stage
        m.heat = c->cat + c->cat_heat; m.paf = paf ? c->cat + PMX_CAT_PAF : nullptr;
        m.sc = 1; m.sx = c->cat_c; m.sy = (long long)c->cur_fw * c->cat_c;
        m.sbh = fhw * c->cat_c; m.sbp = paf ? m.sbh : 0;
    }
    m.fh = c->cur_fh; m.fw = c->cur_fw;
    return m;
}

extern "C" int pmx_postprocess(pmx_ctx* c, int B, int map_h, int map_w, double img_len, const double* scale_xy)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_postprocess: posenet only (use pmx_keypoints for facenet / handnet)");
    PMX_CHECK(c->maps_valid, PMX_ERR_STATE, "pmx_postprocess: no network output (call forward or set_maps first)");
    PMX_CHECK(B == c->cur_B, PMX_ERR_INVALID, "pmx_postprocess: batch %d != batch of the current maps %d", B, c->cur_B);
    PMX_CHECK(c->cur_segs.empty(), PMX_ERR_STATE, "pmx_postprocess: the current maps are those of a mixed-size batch (use pmx_postprocess_images)");
    PMX_CHECK(map_h >= 1 && map_w >= 1 && (long long)map_h * map_w < (1ll << 31), PMX_ERR_INVALID, "pmx_postprocess: bad map size");
    PMX_DEV(c);
    int rc;
    if ((rc = pmx_ensure_tables(c, c->cur_fh, c->cur_fw, map_h, map_w))) return rc;
    const PPMaps m = pmx_current_maps(c);
    if (c->opt_keep_smoothed) {
        if ((rc = pmx_ensure_smoothed(c, (size_t)B * PMX_N_JOINTS * map_h * map_w))) return rc;
    }
    const double* dscale = nullptr;
    if (scale_xy) {
        PMX_HIP(hipMemcpyAsync(c->d_scale, scale_xy, sizeof(double) * 2 * B, hipMemcpyHostToDevice, c->stream));
        dscale = c->d_scale;
    }
    // the candidate scan of a limb over several blocks where the maps come at full resolution (detect_precise, pmx_set_maps: crowds of
    // peaks, 19 blocks per image otherwise); the batch path's low-resolution maps keep the one-block form
    c->pp_limbs_slices = c->opt_limbs_slices >= 0 ? c->opt_limbs_slices : (c->maps_external ? 8 : 0);
    rc = pp_launch(m, c->tab, c->pp, B, map_h, map_w, img_len, dscale, c->opt_keep_smoothed && c->pp.smoothed, c->opt_pp_generic, c->stream,
                   c->prof_on == 1 ? pp_prof_cb : nullptr, c, c->pp_limbs_slices);
    if (rc) return rc;
    c->pp_valid = true; c->pp_final = false; c->pp_B = B; c->pp_h = map_h; c->pp_w = map_w;
    c->pp_maps = m; c->pp_img_len = img_len; c->pp_has_scale = scale_xy != nullptr;
    c->pp_calls.clear();
    return PMX_OK;
}

// the post-process buffers as the images [base, ...) see them: every per-image array moved on by `base` images (strides: pp_alloc)
PPBuffers pmx_pp_view(const PPBuffers& p, int base)
{
    PPBuffers v = p;
    const size_t b = (size_t)base, npk = (size_t)PMX_N_JOINTS * p.cap_pk, nl = (size_t)PMX_N_LIMBS;
    v.pk_raw_key += b * npk; v.pk_raw_score += b * npk; v.pk_count += b * PMX_N_JOINTS;
    v.pk_x += b * npk; v.pk_y += b * npk; v.pk_score += b * npk; v.pk_start += b * (PMX_N_JOINTS + 1);
    v.cn_a += b * nl * p.cap_pk; v.cn_b += b * nl * p.cap_pk; v.cn_score += b * nl * p.cap_pk;
    v.cn_count += b * nl; v.cn_need += b * nl;
    v.scan_score += b * nl * p.scan_cap; v.scan_idx += b * nl * p.scan_cap; v.scan_cnt += b * nl;
    if (p.cand_score) { v.cand_score += b * nl * p.cap_cand; v.cand_idx += b * nl * p.cap_cand; v.cand_used += b * nl * 2 * p.cap_pk; }
    if (p.sub_work) v.sub_work += b * p.cap_sub * 20;
    v.subsets += b * p.cap_sub * 20; v.status += b; v.results += b * p.rec_bytes;
    v.smoothed = nullptr;            // (sized for ONE map size: not available per segment)
    return v;
}

// ---- capacities: the reference has none (np.vstack / lists); ours grow on demand ------------------------------------------
static const int PMX_IMG_CAPACITY_BITS = PMX_IMG_PEAK_OVERFLOW | PMX_IMG_CAND_OVERFLOW | PMX_IMG_SUBSET_OVERFLOW | PMX_IMG_PEOPLE_OVERFLOW;
static int next_pow2(long long v)
{
    long long p = 1;
    while (p < v) p <<= 1;
    return (int)(p > (1ll << 30) ? (1ll << 30) : p);
}

// Synchronise and look at the per-image status words of the last post-process.  If an image overflowed a capacity, grow it
// (peaks: to the largest per-joint count seen; candidates: device-memory store sized to the largest accepted count; subsets:
// doubled), reallocate the post-process buffers and run the post-process of the batch again on the same network output --
// until every image fits.  After this the records on the device are final.
// Re-size the post-process buffers: the new set is allocated FIRST and swapped in only when every allocation succeeded -- on failure (out
// of memory on a crowd image, an absurd user capacity) the context keeps its old buffers and capacities and stays usable
static int pp_realloc(pmx_ctx* c, int cap_pk, int cap_sub, int cap_cand, int cap_ppl)
{
    PPBuffers fresh{};
    DevBuf<char> store;
    fresh.cap_pk = cap_pk; fresh.cap_sub = cap_sub; fresh.cap_cand = cap_cand; fresh.cap_ppl = cap_ppl;
    fresh.smoothed = c->pp.smoothed;             // (c->smoothed, sized separately)
    if (int rc = pp_alloc(fresh, store, c->max_batch)) return rc;
    c->pp = fresh;
    c->pp_store.swap(store);                     // (the old set goes with `store`)
    return PMX_OK;
}

static int pp_finalize(pmx_ctx* c)
{
    if (!c->pp_valid || c->pp_final) return PMX_OK;
    for (int round = 0; round < 64; ++round) {
        const int B = c->pp_B;
        std::vector<int> status(B);
        PMX_HIP(hipMemcpyAsync(status.data(), c->pp.status, sizeof(int) * B, hipMemcpyDeviceToHost, c->stream));
        PMX_HIP(hipStreamSynchronize(c->stream));
        int bits = 0;
        for (int v : status) bits |= v;
        if (!(bits & PMX_IMG_CAPACITY_BITS)) { c->pp_final = true; return PMX_OK; }
        int cap_pk = c->pp.cap_pk, cap_sub = c->pp.cap_sub, cap_cand = c->pp.cap_cand, cap_ppl = c->pp.cap_ppl;
        if (bits & PMX_IMG_PEAK_OVERFLOW) {
            std::vector<int> cnt((size_t)B * PMX_N_JOINTS);
            PMX_HIP(hipMemcpy(cnt.data(), c->pp.pk_count, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
            int need = 0;
            for (int v : cnt) need = v > need ? v : need;
            cap_pk = next_pow2(need);
        }
        if (bits & PMX_IMG_CAND_OVERFLOW) {
            std::vector<int> need_v((size_t)B * PMX_N_LIMBS);
            PMX_HIP(hipMemcpy(need_v.data(), c->pp.cn_need, need_v.size() * sizeof(int), hipMemcpyDeviceToHost));
            int need = PMX_LDS_CANDIDATES;
            for (int v : need_v) need = v > need ? v : need;
            cap_cand = next_pow2(need);
        }
        if (bits & PMX_IMG_SUBSET_OVERFLOW) cap_sub *= 2;
        if (bits & PMX_IMG_PEOPLE_OVERFLOW) {
            int need = 0;
            for (int b = 0; b < B; ++b) {
                pmx_image_info info;
                PMX_HIP(hipMemcpy(&info, c->pp.results + (size_t)b * c->pp.rec_bytes, sizeof info, hipMemcpyDeviceToHost));
                need = info.n_people > need ? info.n_people : need;
            }
            cap_ppl = next_pow2(need);
        }
        // invariant pmx_set_capacities enforces (people <= subsets): keep it through growth, so that a grown state can be replayed
        // through pmx_set_capacities (Engine.state() / load_state() when a PoseDetector re-creates its context)
        if (cap_sub < cap_ppl) cap_sub = cap_ppl;
        PMX_CHECK(cap_pk != c->pp.cap_pk || cap_sub != c->pp.cap_sub || cap_cand != c->pp.cap_cand || cap_ppl != c->pp.cap_ppl,
                  PMX_ERR_STATE, "post-process reports a capacity overflow (0x%x) that growing does not resolve", bits);
        int rc = pp_realloc(c, cap_pk, cap_sub, cap_cand, cap_ppl);
        if (rc) { c->pp_valid = false; return rc; }      // (old buffers and capacities stay in place; this batch has no results)
        c->pp_regrown += 1;
        if (c->pp_calls.empty()) {
            rc = pp_launch(c->pp_maps, c->tab, c->pp, B, c->pp_h, c->pp_w, c->pp_img_len, c->pp_has_scale ? c->d_scale : nullptr,
                           c->opt_keep_smoothed && c->pp.smoothed, c->opt_pp_generic, c->stream, nullptr, nullptr, c->pp_limbs_slices);
        } else {                     // a mixed batch: every segment again, on its own slice of the (new) buffers
            for (const PPCall& q : c->pp_calls)
                if ((rc = pp_launch(q.maps, q.tab, pmx_pp_view(c->pp, q.base), q.B, q.map_h, q.map_w, q.img_len, q.has_scale ? c->d_scale + 2 * q.base : nullptr,
                                    0, c->opt_pp_generic, c->stream, nullptr, nullptr, q.limbs_slices))) break;
        }
        if (rc) { c->pp_valid = false; return rc; }
    }
    pmx_set_error("post-process capacities did not converge");
    return PMX_ERR_STATE;
}

extern "C" int pmx_set_capacities(pmx_ctx* c, int peaks_per_joint, int subsets, int people, int candidates)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(peaks_per_joint >= 0 && subsets >= 0 && people >= 0 && candidates >= 0, PMX_ERR_INVALID, "pmx_set_capacities: negative capacity");
    const int lim = 1 << 20;
    PMX_CHECK(peaks_per_joint <= lim && subsets <= lim && people <= lim && candidates <= (1 << 24), PMX_ERR_INVALID, "pmx_set_capacities: capacity too large");
    const int cap_pk = peaks_per_joint ? peaks_per_joint : c->pp.cap_pk, cap_sub = subsets ? subsets : c->pp.cap_sub;
    const int cap_ppl = people ? people : c->pp.cap_ppl;
    PMX_CHECK(cap_ppl <= cap_sub, PMX_ERR_INVALID, "pmx_set_capacities: people (%d) must not exceed subsets (%d)", cap_ppl, cap_sub);
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    c->pp_valid = false;
    return pp_realloc(c, cap_pk, cap_sub, candidates, cap_ppl);
}

extern "C" int pmx_get_capacities(pmx_ctx* c, int* peaks_per_joint, int* subsets, int* people, int* candidates)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    if (peaks_per_joint) *peaks_per_joint = c->pp.cap_pk;
    if (subsets) *subsets = c->pp.cap_sub;
    if (people) *people = c->pp.cap_ppl;
    if (candidates) *candidates = c->pp.cap_cand;
    return PMX_OK;
}

// Does pmx_detect_batch run this batch as two half-batch chains (option "batch_chains"; pmx_ctx.h: BatchChain)?  Only a uniform fp32 inference
// batch of the pose network; then a probe walks the forward without launching anything: no layer cut in two by images, every launch of a
// half the launch its whole-batch plan describes, and -- the automatic rule, under conv_algo 1 -- the halves of every 7x7 plain launch whole
// rounds of the CUs.  The verdict is kept per (B, H, W) until an option changes.
static int chains_wanted(pmx_ctx* c, const uint8_t* d, int B, int H, int W, bool* yes)
{
    *yes = false;
    if (!c->opt_batch_chains || B < 2 || c->kind != NET_POSE || c->opt_precision != 0 || c->ls_on || c->bw.on || c->tr.on || c->opt_keep_smoothed) return PMX_OK;
    // (automatic: not under the per-launch profiler -- its event pairs would time a launch's wait for CUs the other chain holds, and its
    //  labels are the one plan per layer that the C twin reads; the 7x7-only profile of timed regions keeps the form that is being timed)
    if (c->opt_batch_chains < 0 && (c->opt_conv_algo != 1 || c->prof_on == 1)) return PMX_OK;
    const int key[4] = {B, H, W, c->opt_epoch};
    if (memcmp(key, c->chains_key, sizeof key)) {
        ChainSplit s;
        s.n0 = B / 2; s.probe = true;
        FwdCall k = pmx_call(c);
        k.split = &s;
        c->chains_key[3] = -1;
        if (int rc = pmx_forward_from_u8(c, k, d, B, H, W, 255.0f)) return rc;
        memcpy(c->chains_key, key, sizeof key);
        c->chains_ok = s.ok; c->chains_rounds = s.rounds;
    }
    *yes = c->chains_ok && (c->opt_batch_chains > 0 || c->chains_rounds);
    return PMX_OK;
}

// The batch as two chains: images [0, n0) on the context's stream, [n0, B) on the second stream, forked here and joined before the return --
// network and post-process of a half never wait for the other half, and whatever is enqueued on the context's stream afterwards sees the
// records of all B images.  No host synchronisation beyond what the one-chain call has (the tables of a new map size, buffers that grow).
static int detect_batch_chains(pmx_ctx* c, const uint8_t* d, int B, int H, int W, int map_h, int map_w, double img_len, const double* scale_xy)
{
    BatchChain& ch = c->chain2;
    int rc;
    if ((rc = ch.stream.create(hipStreamNonBlocking)) || (rc = ch.fork.create(hipEventDisableTiming)) || (rc = ch.done.create(hipEventDisableTiming))) return rc;
    if ((rc = pmx_ensure_tables(c, H / 8, W / 8, map_h, map_w))) return rc;
    const double* dscale = nullptr;
    if (scale_xy) {
        PMX_HIP(hipMemcpyAsync(c->d_scale, scale_xy, sizeof(double) * 2 * B, hipMemcpyHostToDevice, c->stream));
        dscale = c->d_scale;
    }
    PMX_HIP(hipEventRecord(ch.fork, c->stream));
    PMX_HIP(hipStreamWaitEvent(ch.stream, ch.fork, 0));
    ChainSplit s;
    s.n0 = B / 2; s.net_px = (size_t)H * W; s.second = &ch;
    FwdCall k = pmx_call(c);
    k.split = &s;
    rc = pmx_forward_from_u8(c, k, d, B, H, W, 255.0f);
    const PPMaps m = pmx_current_maps(c);
    c->pp_limbs_slices = c->opt_limbs_slices >= 0 ? c->opt_limbs_slices : 0;
    struct ProfCtx { pmx_ctx* c; const LaunchPart& part; };
    auto prof_cb = [](void* v, const char* name, int begin) {
        ProfCtx* p = (ProfCtx*)v;
        if (begin) (void)prof_begin(p->c, p->part.k, std::string(name) + "|" + name + p->part.suffix, 0, 0);
        else (void)prof_end(p->c, p->part.k);
    };
    if (!rc) rc = for_each_part(k, B, [&](const LaunchPart& part) {
        ProfCtx pc{c, part};
        PPMaps mi = m;
        mi.heat += part.first * m.sbh; mi.paf += part.first * m.sbp;
        return pp_launch(mi, c->tab, pmx_pp_view(c->pp, part.first), part.n, map_h, map_w, img_len, dscale ? dscale + 2 * part.first : nullptr, 0, c->opt_pp_generic,
                         part.k.stream, c->prof_on == 1 ? +prof_cb : nullptr, &pc, c->pp_limbs_slices);
    });
    // the join, whatever happened in between: the context's stream never runs ahead of the second chain
    PMX_HIP(hipEventRecord(ch.done, ch.stream));
    PMX_HIP(hipStreamWaitEvent(c->stream, ch.done, 0));
    if (rc) return rc;
    c->pp_valid = true; c->pp_final = false; c->pp_B = B; c->pp_h = map_h; c->pp_w = map_w;
    c->pp_maps = m; c->pp_img_len = img_len; c->pp_has_scale = scale_xy != nullptr;
    c->pp_calls.clear();
    return PMX_OK;
}

extern "C" int pmx_detect_batch(pmx_ctx* c, const uint8_t* img, int B, int H, int W, int on_device, int map_h, int map_w,
                                double img_len, const double* scale_xy)
{
    bool chains = false;
    if (c && img && c->opt_batch_chains && map_h >= 1 && map_w >= 1 && (long long)map_h * map_w < (1ll << 31)) {
        int rc = check_forward_args(c, img, B, H, W);
        if (rc) return rc;
        PMX_DEV(c);
        if ((rc = chains_wanted(c, img, B, H, W, &chains))) return rc;
        if (chains) {
            const uint8_t* d = img;
            if (!on_device) {
                PMX_HIP(hipMemcpyAsync(c->u8_tmp, img, (size_t)B * H * W * 3, hipMemcpyHostToDevice, c->stream));
                d = c->u8_tmp;
            }
            return detect_batch_chains(c, d, B, H, W, map_h, map_w, img_len, scale_xy);
        }
    }
    int rc = pmx_forward_u8(c, img, B, H, W, on_device);
    if (rc) return rc;
    return pmx_postprocess(c, B, map_h, map_w, img_len, scale_xy);
}

extern "C" int pmx_results_layout(pmx_ctx* c, int* people_cap, size_t* bytes_per_record)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->pp_valid, PMX_ERR_STATE, "pmx_results_layout: no post-process results yet");
    PMX_DEV(c);
    int rc = pp_finalize(c);
    if (rc) return rc;
    if (people_cap) *people_cap = c->pp.cap_ppl;
    if (bytes_per_record) *bytes_per_record = c->pp.rec_bytes;
    return PMX_OK;
}

extern "C" int pmx_get_results(pmx_ctx* c, int B, void* out, size_t out_bytes)
{
    PMX_CHECK(c && out, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(c->pp_valid && B >= 1 && B <= c->pp_B, PMX_ERR_STATE, "pmx_get_results: no post-process results for batch %d", B);
    PMX_DEV(c);
    for (;;) {
        const size_t rec = c->pp.rec_bytes, need = rec * (size_t)B;
        PMX_CHECK(out_bytes >= need, PMX_ERR_CAPACITY, "pmx_get_results: %zu bytes for %d records of %zu bytes (see pmx_results_layout)",
                  out_bytes, B, rec);
        if (need > c->h_results.capacity())
            if (int rc = c->h_results.alloc(rec * (size_t)c->max_batch)) return rc;
        PMX_HIP(hipMemcpyAsync(c->h_results, c->pp.results, need, hipMemcpyDeviceToHost, c->stream));
        PMX_HIP(hipStreamSynchronize(c->stream));
        if (!c->pp_final) {
            // common case: the records just copied carry the status words -- no extra round trip
            int bits = 0;
            for (int b = 0; b < B; ++b) bits |= reinterpret_cast<const pmx_image_info*>(c->h_results + (size_t)b * rec)->status;
            if (B == c->pp_B && !(bits & PMX_IMG_CAPACITY_BITS)) c->pp_final = true;
            else {
                int rc = pp_finalize(c);        // grows + re-runs if needed; the record layout may have changed
                if (rc) return rc;
                continue;
            }
        }
        memcpy(out, c->h_results, need);
        return PMX_OK;
    }
}

extern "C" int pmx_results_device_ptr(pmx_ctx* c, void** p, size_t* bytes)
{
    PMX_CHECK(c && p && bytes, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(c->pp_valid, PMX_ERR_STATE, "no post-process results yet");
    if (hipSetDevice(c->device) != hipSuccess) { pmx_set_error("hipSetDevice failed"); return PMX_ERR_HIP; }
    if (int rc = pp_finalize(c)) return rc;      // never hand out records that still carry capacity-overflow bits / a layout about to change
    *p = c->pp.results;
    *bytes = c->pp.rec_bytes;
    return PMX_OK;
}

extern "C" int pmx_results_snapshot(pmx_ctx* c, int slot, void* dst_device, size_t dst_bytes)
{
    PMX_CHECK(c && dst_device, PMX_ERR_INVALID, "null arg");
    PMX_CHECK(slot >= 0 && slot < PMX_SNAPSHOT_SLOTS, PMX_ERR_INVALID, "pmx_results_snapshot: slot %d outside 0..%d", slot, PMX_SNAPSHOT_SLOTS - 1);
    PMX_CHECK(c->pp_valid, PMX_ERR_STATE, "pmx_results_snapshot: no post-process results yet");
    PMX_DEV(c);
    const size_t need = c->pp.rec_bytes * (size_t)c->pp_B;
    PMX_CHECK(dst_bytes >= need, PMX_ERR_CAPACITY, "pmx_results_snapshot: %zu bytes for %d records of %zu bytes", dst_bytes, c->pp_B, c->pp.rec_bytes);
    if (int rc = c->snap_ev[slot].create(hipEventDisableTiming)) return rc;
    if (!c->snap_status[slot])
        if (int rc = c->snap_status[slot].alloc(c->max_batch)) return rc;
    PMX_HIP(hipMemcpyAsync(dst_device, c->pp.results, need, hipMemcpyDeviceToDevice, c->stream));
    PMX_HIP(hipMemcpyAsync(c->snap_status[slot], c->pp.status, sizeof(int) * (size_t)c->pp_B, hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipEventRecord(c->snap_ev[slot], c->stream));
    c->snap_B[slot] = c->pp_B; c->snap_cap_ppl[slot] = c->pp.cap_ppl; c->snap_rec[slot] = c->pp.rec_bytes;
    return PMX_OK;
}

extern "C" int pmx_snapshot_wait(pmx_ctx* c, int slot, int* batch, int* people_cap, size_t* bytes_per_record, int* status_or)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(slot >= 0 && slot < PMX_SNAPSHOT_SLOTS && c->snap_ev[slot] && c->snap_B[slot] > 0, PMX_ERR_STATE, "pmx_snapshot_wait: slot %d holds no snapshot", slot);
    PMX_DEV(c);
    PMX_HIP(hipEventSynchronize(c->snap_ev[slot]));
    int bits = 0;
    for (int b = 0; b < c->snap_B[slot]; ++b) bits |= c->snap_status[slot][b];
    if (batch) *batch = c->snap_B[slot];
    if (people_cap) *people_cap = c->snap_cap_ppl[slot];
    if (bytes_per_record) *bytes_per_record = c->snap_rec[slot];
    if (status_or) *status_or = bits;
    return PMX_OK;
}

static int check_pp_image(pmx_ctx* c, int image)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(c->pp_valid, PMX_ERR_STATE, "no post-process results yet");
    PMX_CHECK(image >= 0 && image < c->pp_B, PMX_ERR_INVALID, "image %d outside 0..%d", image, c->pp_B - 1);
    if (hipSetDevice(c->device) != hipSuccess) { pmx_set_error("hipSetDevice failed"); return PMX_ERR_HIP; }
    return pp_finalize(c);
}

extern "C" int pmx_get_peaks(pmx_ctx* c, int image, double* peaks5, int cap, int* n_rows)
{
    int rc = check_pp_image(c, image);
    if (rc) return rc;
    PMX_CHECK(peaks5 && n_rows, PMX_ERR_INVALID, "null arg");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    int start[PMX_N_JOINTS + 1];
    PMX_HIP(hipMemcpy(start, c->pp.pk_start + image * (PMX_N_JOINTS + 1), sizeof start, hipMemcpyDeviceToHost));
    const int n = start[PMX_N_JOINTS];
    *n_rows = n;
    PMX_CHECK(n <= cap, PMX_ERR_CAPACITY, "pmx_get_peaks: %d rows > capacity %d", n, cap);
    std::vector<int> x(n), y(n);
    std::vector<float> s(n);
    if (n) {
        const size_t pbase = (size_t)image * PMX_N_JOINTS * c->pp.cap_pk;
        PMX_HIP(hipMemcpy(x.data(), c->pp.pk_x + pbase, n * sizeof(int), hipMemcpyDeviceToHost));
        PMX_HIP(hipMemcpy(y.data(), c->pp.pk_y + pbase, n * sizeof(int), hipMemcpyDeviceToHost));
        PMX_HIP(hipMemcpy(s.data(), c->pp.pk_score + pbase, n * sizeof(float), hipMemcpyDeviceToHost));
    }
    int j = 0;
    for (int i = 0; i < n; ++i) {
        while (j < PMX_N_JOINTS && i >= start[j + 1]) ++j;
        peaks5[i * 5 + 0] = j; peaks5[i * 5 + 1] = x[i]; peaks5[i * 5 + 2] = y[i]; peaks5[i * 5 + 3] = (double)s[i]; peaks5[i * 5 + 4] = i;
    }
    return PMX_OK;
}

extern "C" int pmx_get_connections(pmx_ctx* c, int image, double* conns4, int cap, int* n_rows)
{
    int rc = check_pp_image(c, image);
    if (rc) return rc;
    PMX_CHECK(conns4 && n_rows, PMX_ERR_INVALID, "null arg");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    int cnt[PMX_N_LIMBS];
    PMX_HIP(hipMemcpy(cnt, c->pp.cn_count + image * PMX_N_LIMBS, sizeof cnt, hipMemcpyDeviceToHost));
    int total = 0;
    for (int l = 0; l < PMX_N_LIMBS; ++l) total += cnt[l];
    *n_rows = total;
    PMX_CHECK(total <= cap, PMX_ERR_CAPACITY, "pmx_get_connections: %d rows > capacity %d", total, cap);
    int o = 0;
    const int cap_pk = c->pp.cap_pk;
    std::vector<int> a(cap_pk), b(cap_pk);
    std::vector<double> s(cap_pk);
    for (int l = 0; l < PMX_N_LIMBS; ++l) {
        const int n = cnt[l];
        if (!n) continue;
        const size_t base = ((size_t)image * PMX_N_LIMBS + l) * cap_pk;
        PMX_HIP(hipMemcpy(a.data(), c->pp.cn_a + base, n * sizeof(int), hipMemcpyDeviceToHost));
        PMX_HIP(hipMemcpy(b.data(), c->pp.cn_b + base, n * sizeof(int), hipMemcpyDeviceToHost));
        PMX_HIP(hipMemcpy(s.data(), c->pp.cn_score + base, n * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i, ++o) {
            conns4[o * 4 + 0] = l; conns4[o * 4 + 1] = a[i]; conns4[o * 4 + 2] = b[i]; conns4[o * 4 + 3] = s[i];
        }
    }
    return PMX_OK;
}

extern "C" int pmx_get_subsets(pmx_ctx* c, int image, double* subsets20, int cap, int* n_rows)
{
    int rc = check_pp_image(c, image);
    if (rc) return rc;
    PMX_CHECK(subsets20 && n_rows, PMX_ERR_INVALID, "null arg");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    pmx_image_info info;
    PMX_HIP(hipMemcpy(&info, c->pp.results + (size_t)image * c->pp.rec_bytes, sizeof info, hipMemcpyDeviceToHost));
    int n = info.n_people;      // rows kept by the final filter
    *n_rows = n;
    PMX_CHECK(n <= cap, PMX_ERR_CAPACITY, "pmx_get_subsets: %d rows > capacity %d", n, cap);
    if (n) PMX_HIP(hipMemcpy(subsets20, c->pp.subsets + (size_t)image * c->pp.cap_sub * 20, (size_t)n * 20 * sizeof(double),
                             hipMemcpyDeviceToHost));
    return PMX_OK;
}

extern "C" int pmx_get_smoothed(pmx_ctx* c, int image, int joint, float* out, int map_h, int map_w)
{
    int rc = check_pp_image(c, image);
    if (rc) return rc;
    const int n_ch = c->kind == NET_POSE ? PMX_N_JOINTS : c->n_heat - 1;
    PMX_CHECK(out && joint >= 0 && joint < n_ch, PMX_ERR_INVALID, "bad arg");
    PMX_CHECK(c->pp.smoothed && (c->opt_keep_smoothed || c->kind != NET_POSE), PMX_ERR_STATE, "pmx_get_smoothed: option keep_smoothed was not set");
    PMX_CHECK(map_h == c->pp_h && map_w == c->pp_w, PMX_ERR_INVALID, "pmx_get_smoothed: map size mismatch");
    PMX_DEV(c);
    PMX_HIP(hipStreamSynchronize(c->stream));
    PMX_HIP(hipMemcpy(out, c->pp.smoothed + ((size_t)image * n_ch + joint) * map_h * map_w, (size_t)map_h * map_w * sizeof(float),
                      hipMemcpyDeviceToHost));
    return PMX_OK;
}

// ------------------------------------------------------------------------------------- measurement
extern "C" int pmx_timer_start(pmx_ctx* c)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_DEV(c);
    PMX_HIP(hipEventRecord(c->t0, c->stream));
    return PMX_OK;
}
extern "C" int pmx_timer_stop(pmx_ctx* c, double* ms)
{
    PMX_CHECK(c && ms, PMX_ERR_INVALID, "null arg");
    PMX_DEV(c);
    PMX_HIP(hipEventRecord(c->t1, c->stream));
    PMX_HIP(hipEventSynchronize(c->t1));
    float f = 0.f;
    PMX_HIP(hipEventElapsedTime(&f, c->t0, c->t1));
    *ms = f;
    return PMX_OK;
}
extern "C" int pmx_profile_enable(pmx_ctx* c, int on)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_DEV(c);
    int rc = prof_collect(c);
    c->prof_on = on < 0 ? 0 : (on > 2 ? 1 : on);
    return rc;
}
extern "C" int pmx_profile_reset(pmx_ctx* c)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_DEV(c);
    int rc = prof_collect(c);
    c->prof.clear();
    c->prof_index.clear();
    return rc;
}
extern "C" int pmx_profile_count(pmx_ctx* c, int* n)
{
    PMX_CHECK(c && n, PMX_ERR_INVALID, "null arg");
    PMX_DEV(c);
    int rc = prof_collect(c);
    *n = (int)c->prof.size();
    return rc;
}
extern "C" int pmx_profile_issued(pmx_ctx* c, int i, double* issued_flop)
{
    PMX_CHECK(c && issued_flop && i >= 0 && i < (int)c->prof.size(), PMX_ERR_INVALID, "bad profile index");
    *issued_flop = c->prof[i].issued;
    return PMX_OK;
}

extern "C" int pmx_profile_entry(pmx_ctx* c, int i, char* name, int cap, double* total_ms, int64_t* launches, double* flops, double* bytes)
{
    PMX_CHECK(c && i >= 0 && i < (int)c->prof.size(), PMX_ERR_INVALID, "bad profile index");
    const ProfEntry& e = c->prof[i];
    if (name && cap > 0) { strncpy(name, e.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (total_ms) *total_ms = e.total_ms;
    if (launches) *launches = e.launches;
    if (flops) *flops = e.flops;
    if (bytes) *bytes = e.bytes;
    return PMX_OK;
}

// ---------------------------------------------------------------------------- single-layer test entries
// a layer that is not in the context's table: packed as set_layer packs one (identity channel map); its buffers, derived packs included,
// are freed with it
static int test_layer(pmx_ctx* c, PackedLayer& L, const float* w, const float* bias, int cout, int cin, int ks)
{
    DevBuf<float> master;
    int rc;
    if ((rc = master.alloc((size_t)cout * cin * ks * ks + cout)) || (rc = upload_master(master, w, bias, cout, cin, ks, c->stream))) return rc;
    pmx_layer_geometry(L, cout, cin, ks, pmx_pk_cin_pad(0, cin));
    if ((rc = build_direct(L, 0, master, c->stream))) return rc;
    L.set = true;
    return PMX_OK;
}
// host NCHW x -> channels [coff, coff + cin) of the NHWC buffer d_xn (channel stride lda), through the staging buffer d_x
static int test_upload(pmx_ctx* c, const float* x, DevBuf<float>& d_x, float* d_xn, int B, int cin, int H, int W, int lda, int coff)
{
    PMX_HIP(hipMemcpy(d_x, x, (size_t)B * cin * H * W * 4, hipMemcpyHostToDevice));
    return launch_nchw_to_nhwc(d_x, d_xn, B, cin, H, W, lda, coff, c->stream);
}
// channels [coff, coff + cout) of the NHWC result d_yn (channel stride ldc) -> host NCHW y, through the staging buffer d_y; synchronises
static int test_fetch(pmx_ctx* c, const char* who, const float* d_yn, DevBuf<float>& d_y, float* y, int B, int cout, int Ho, int Wo, int ldc, int coff)
{
    int rc = launch_nhwc_to_nchw(d_yn, d_y, B, cout, Ho, Wo, ldc, coff, c->stream);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(y, d_y, (size_t)B * cout * Ho * Wo * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { pmx_set_error("%s: %s", who, hipGetErrorString(e)); return PMX_ERR_HIP; }
    return PMX_OK;
}

// One layer that is not in the context's table, through the dispatcher of the network (plan_conv + launch_plan) under the context's options:
// the whole batch as ONE plan (no cut by images), never profiled; avg_ms = `iters` launches of that plan between two events.
extern "C" int pmx_conv2d(pmx_ctx* c, const float* x, const float* w, const float* bias, int B, int cin, int H, int W, int cout,
                          int ks, int relu, int pool, float* y, int iters, double* avg_ms)
{
    PMX_CHECK(c && x && w && y, PMX_ERR_INVALID, "pmx_conv2d: null arg");
    PMX_CHECK(ks == 1 || ks == 3 || ks == 7, PMX_ERR_INVALID, "pmx_conv2d: ksize must be 1, 3 or 7");
    PMX_CHECK(B >= 1 && cin >= 1 && cout >= 1 && H >= 1 && W >= 1, PMX_ERR_INVALID, "pmx_conv2d: bad shape");
    PMX_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), PMX_ERR_INVALID, "pmx_conv2d: pool needs even H, W");
    PMX_DEV(c);
    PackedLayer L;
    int rc;
    if ((rc = test_layer(c, L, w, bias, cout, cin, ks))) return rc;
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    DevBuf<float> d_x, d_xn, d_y, d_yn;
    const size_t nx = (size_t)B * cin * H * W, nxn = (size_t)B * H * W * L.cin_pad, ny = (size_t)B * cout * Ho * Wo;
    if ((rc = d_x.alloc(nx)) || (rc = d_xn.alloc(nxn)) || (rc = d_y.alloc(ny)) || (rc = d_yn.alloc(ny))) return rc;
    PMX_HIP(hipMemsetAsync(d_xn, 0, nxn * 4, c->stream));
    // poison the output so that unwritten elements are caught by the test
    PMX_HIP(hipMemsetAsync(d_yn, 0xFF, ny * 4, c->stream));
    if ((rc = test_upload(c, x, d_x, d_xn, B, cin, H, W, L.cin_pad, 0))) return rc;
    const FwdCall k = pmx_call(c);
    ConvPlan p;
    if ((rc = plan_conv(c, k, p, nullptr, &L, nullptr, conv_io(ConvBuf::one(d_xn, L.cin_pad), ConvBuf::one(d_yn, cout), B, H, W, relu, pool)))) return rc;
    rc = launch_plan(c, k, p);
    if (!rc && iters > 0) {
        Event e0, e1;
        if ((rc = e0.create(hipEventDefault)) || (rc = e1.create(hipEventDefault))) return rc;
        PMX_HIP(hipEventRecord(e0, c->stream));
        for (int i = 0; i < iters && !rc; ++i) rc = launch_plan(c, k, p);
        PMX_HIP(hipEventRecord(e1, c->stream));
        PMX_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        PMX_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (avg_ms) *avg_ms = ms / iters;
    }
    return rc ? rc : test_fetch(c, "pmx_conv2d", d_yn, d_y, y, B, cout, Ho, Wo, cout, 0);
}

// pmx_conv2d for two layers as the two groups of ONE plan (include/pose_mi355x.h), laid out the way run_conv's callers lay out the L1 / L2
// branches: both inputs are channel slices of one NHWC buffer, both outputs channel slices of another, with channels of nobody between
// and after them.  x1 null: both groups read x0's slice.
extern "C" int pmx_conv2d_pair(pmx_ctx* c, const float* x0, const float* x1, const float* w0, const float* bias0, int cout0, const float* w1,
                               const float* bias1, int cout1, int B, int cin, int H, int W, int ks, int relu, int pool, float* y0, float* y1)
{
    PMX_CHECK(c && x0 && w0 && w1 && y0 && y1, PMX_ERR_INVALID, "pmx_conv2d_pair: null arg");
    PMX_CHECK(ks == 1 || ks == 3 || ks == 7, PMX_ERR_INVALID, "pmx_conv2d_pair: ksize must be 1, 3 or 7");
    PMX_CHECK(B >= 1 && cin >= 1 && cout0 >= 1 && cout1 >= 1 && H >= 1 && W >= 1, PMX_ERR_INVALID, "pmx_conv2d_pair: bad shape");
    PMX_CHECK(cout_pad_of(cout0) == cout_pad_of(cout1), PMX_ERR_INVALID, "pmx_conv2d_pair: %d and %d output channels do not pad to the same count",
              cout0, cout1);
    PMX_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), PMX_ERR_INVALID, "pmx_conv2d_pair: pool needs even H, W");
    PMX_DEV(c);
    PackedLayer L[2];
    int rc;
    if ((rc = test_layer(c, L[0], w0, bias0, cout0, cin, ks)) || (rc = test_layer(c, L[1], w1, bias1, cout1, cin, ks))) return rc;
    const int cin_pad = L[0].cin_pad, Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W;
    // input slices at channels 16 and 16 + cin_pad of lda, output slices at 0 and cout0 (rounded up to 4) of ldc: 4 channels of nobody at the end
    const int ioff[2] = {CK, x1 ? CK + cin_pad : CK}, lda = ioff[1] + cin_pad + CK;
    const int ooff[2] = {0, round_up(cout0, 4)}, ldc = ooff[1] + round_up(cout1, 4) + 4, cmax = std::max(cout0, cout1);
    DevBuf<float> d_x, d_xn, d_y, d_yn;
    const size_t nx = (size_t)B * cin * H * W, nxn = (size_t)B * H * W * lda, ny = (size_t)B * cmax * Ho * Wo, nyn = (size_t)B * Ho * Wo * ldc;
    if ((rc = d_x.alloc(nx)) || (rc = d_xn.alloc(nxn)) || (rc = d_y.alloc(ny)) || (rc = d_yn.alloc(nyn))) return rc;
    PMX_HIP(hipMemsetAsync(d_xn, 0, nxn * 4, c->stream));
    PMX_HIP(hipMemsetAsync(d_yn, 0xFF, nyn * 4, c->stream));                    // poison, as in pmx_conv2d
    if ((rc = test_upload(c, x0, d_x, d_xn, B, cin, H, W, lda, ioff[0]))) return rc;
    if (x1) {
        PMX_HIP(hipStreamSynchronize(c->stream));                               // (d_x is staged into again)
        if ((rc = test_upload(c, x1, d_x, d_xn, B, cin, H, W, lda, ioff[1]))) return rc;
    }
    const FwdCall k = pmx_call(c);
    ConvPlan p;
    if ((rc = plan_conv(c, k, p, nullptr, &L[0], &L[1], conv_io(ConvBuf::two(d_xn.get() + ioff[0], ioff[1] - ioff[0], lda), ConvBuf::two(d_yn.get(), ooff[1], ldc),
                                                           B, H, W, relu, pool)))) return rc;
    if ((rc = launch_plan(c, k, p))) return rc;
    if ((rc = test_fetch(c, "pmx_conv2d_pair", d_yn, d_y, y0, B, cout0, Ho, Wo, ldc, ooff[0]))) return rc;
    return test_fetch(c, "pmx_conv2d_pair", d_yn, d_y, y1, B, cout1, Ho, Wo, ldc, ooff[1]);
}

// The backward twin of pmx_conv2d (include/pose_mi355x.h).  z and dx are plans of the dispatcher, each the whole batch as ONE plan as in
// pmx_conv2d; the mask, the bias gradient and the weight gradient are conv_bwd.hip's launches.  Every buffer is a DevBuf or lives in a
// PackedLayer: freed on every way out.
extern "C" int pmx_conv2d_backward(pmx_ctx* c, const float* x, const float* w, const float* bias, const float* dy, int B, int cin, int H, int W,
                                   int cout, int ks, int relu, int pool, float* dx, float* dw, float* db, float* z, int iters, double* avg_ms3)
{
    PMX_CHECK(c && x && w && dy, PMX_ERR_INVALID, "pmx_conv2d_backward: null x, w or dy");
    PMX_CHECK(dx || dw || db || z, PMX_ERR_INVALID, "pmx_conv2d_backward: all four outputs are NULL");
    PMX_CHECK(ks == 1 || ks == 3 || ks == 7, PMX_ERR_INVALID, "pmx_conv2d_backward: ksize must be 1, 3 or 7");
    PMX_CHECK(B >= 1 && cin >= 1 && cout >= 1 && H >= 1 && W >= 1, PMX_ERR_INVALID, "pmx_conv2d_backward: bad shape");
    PMX_CHECK(!pool || (H % 2 == 0 && W % 2 == 0), PMX_ERR_INVALID, "pmx_conv2d_backward: pool needs even H, W");
    PMX_CHECK(c->opt_precision == 0, PMX_ERR_STATE,
              "pmx_conv2d_backward: option \"precision\" is %d; the gradients are fp32 only (the f16 and bf16x3 modes are inference modes)", c->opt_precision);
    PMX_DEV(c);
    const bool need_z = z || relu || pool, need_g = dx || dw || db;
    const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, cg = round_up(cout, 32), cx = round_up(cin, 32), T = ks * ks;
    const size_t npix = (size_t)B * H * W, nx = npix * cin, nz = npix * cout, ndy = (size_t)B * cout * Ho * Wo, ndw = (size_t)cout * cin * T;
    if (avg_ms3) avg_ms3[0] = avg_ms3[1] = avg_ms3[2] = 0.0;
    // L: the layer itself (z); Lt: the layer whose forward is the data gradient
    PackedLayer L, Lt;
    DevBuf<float> d_x, d_xn, d_x32, d_zn, d_z, d_dy, d_g, d_dxn, d_dx, d_ws, d_dw, d_db;
    DevBuf<double> d_part;
    int rc;
    if ((rc = d_x.alloc(nx))) return rc;
    PMX_HIP(hipMemcpy(d_x, x, nx * 4, hipMemcpyHostToDevice));
    auto to_nhwc = [&](DevBuf<float>& dst, int ld) -> int {      // x as NHWC with ld channels per pixel, the padding channels zero
        if (int r = dst.alloc(npix * ld)) return r;
        PMX_HIP(hipMemsetAsync(dst, 0, npix * ld * 4, c->stream));
        return launch_nchw_to_nhwc(d_x, dst, B, cin, H, W, ld, 0, c->stream);
    };
    // option "grad_precision" = 2: dw and dx of a 3x3 / 7x7 layer with f16 operands; z (k) stays under the context's own precision
    const bool f16 = c->opt_grad_precision == 2 && ks > 1;
    const FwdCall k = pmx_call(c);
    FwdCall kt = k;
    if (f16) kt.precision = 2;
    ConvPlan pz, pt;
    if (need_z) {
        if ((rc = test_layer(c, L, w, bias, cout, cin, ks)) || (rc = to_nhwc(d_xn, L.cin_pad)) || (rc = d_zn.alloc(nz))) return rc;
        PMX_HIP(hipMemsetAsync(d_zn, 0xFF, nz * 4, c->stream));
        if ((rc = plan_conv(c, k, pz, nullptr, &L, nullptr, conv_io(ConvBuf::one(d_xn, L.cin_pad), ConvBuf::one(d_zn, cout), B, H, W, 0, 0)))) return rc;
        if ((rc = launch_plan(c, k, pz))) return rc;
    }
    if (need_g) {
        if ((rc = d_dy.alloc(ndy)) || (rc = d_g.alloc(npix * cg))) return rc;
        PMX_HIP(hipMemcpy(d_dy, dy, ndy * 4, hipMemcpyHostToDevice));
    }
    if (db && ((rc = d_part.alloc((size_t)PMX_DB_SLOTS * cg)) || (rc = d_db.alloc(cout)))) return rc;
    if (dx) {
        // (its input padding is its own: g has only cg channels per pixel, so cout rounded up to 16 and not pmx_pk_t_cin_pad's 64 at least)
        DevBuf<float> master;
        if ((rc = master.alloc(ndw + cout)) || (rc = upload_master(master, w, nullptr, cout, cin, ks, c->stream))) return rc;
        pmx_layer_geometry(Lt, cin, cout, ks, round_up(cout, CK));
        if ((rc = build_transposed(Lt, cout, cin, ks, 0, master, c->stream)) || (rc = d_dxn.alloc(nx)) || (rc = d_dx.alloc(nx))) return rc;
        Lt.set = true;
        PMX_HIP(hipMemsetAsync(d_dxn, 0xFF, nx * 4, c->stream));       // poison: an unwritten element is caught by the test
        // g has cg >= Lt.cin_pad channels per pixel, the padding channels zero
        if ((rc = plan_conv(c, kt, pt, nullptr, &Lt, nullptr, conv_io(ConvBuf::one(d_g, cg), ConvBuf::one(d_dxn, cin), B, H, W, 0, 0)))) return rc;
    }
    int strips = 0, rows = 0;
    if (dw) {
        strips = f16 ? conv_wgrad_f16_strips(B, H, cg, cx, ks, c->opt_wgrad_strips, &rows) : conv_wgrad_strips(B, H, cg, cx, ks, c->opt_wgrad_strips, &rows);
        if ((rc = to_nhwc(d_x32, cx)) || (rc = d_ws.alloc((size_t)strips * T * cg * cx)) || (rc = d_dw.alloc(ndw))) return rc;
        PMX_HIP(hipMemsetAsync(d_dw, 0xFF, ndw * 4, c->stream));
    }
    // the three parts; each is timed on its own between two events
    auto mask_db = [&]() -> int {
        if (!need_g) return PMX_OK;
        if (int r = conv_bwd_mask_launch(d_dy, d_zn, cout, d_g, B, H, W, cout, cg, relu, pool, c->stream)) return r;
        return db ? conv_bwd_db_launch(d_g, cg, d_part, d_db, (long long)npix, cout, cg, c->stream) : PMX_OK;
    };
    auto data_grad = [&]() -> int { return dx ? launch_plan(c, kt, pt) : PMX_OK; };
    auto weight_grad = [&]() -> int {
        if (!dw) return PMX_OK;
        return (f16 ? conv_wgrad_f16_launch : conv_wgrad_launch)(d_g, cg, d_x32, cx, d_ws, d_dw, B, H, W, cout, cg, cin, cx, ks, strips, rows, nullptr, c->stream,
                                                                 PMX_WGRAD_MAX_STRIPS);
    };
    Event e0, e1;
    auto timed = [&](const std::function<int()>& part, double* ms_out) -> int {
        PMX_HIP(hipEventRecord(e0, c->stream));
        int r = PMX_OK;
        for (int i = 0; i < iters && !r; ++i) r = part();
        PMX_HIP(hipEventRecord(e1, c->stream));
        PMX_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        PMX_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (ms_out) *ms_out = ms / iters;
        return r;
    };
    auto run = [&]() -> int {
        int r;
        if ((r = mask_db()) || (r = data_grad()) || (r = weight_grad())) return r;
        if (iters > 0) {
            if ((r = e0.create(hipEventDefault)) || (r = e1.create(hipEventDefault))) return r;
            if (dx && (r = timed(data_grad, avg_ms3 ? avg_ms3 + 0 : nullptr))) return r;
            if (dw && (r = timed(weight_grad, avg_ms3 ? avg_ms3 + 1 : nullptr))) return r;
            if (need_g && (r = timed(mask_db, avg_ms3 ? avg_ms3 + 2 : nullptr))) return r;
        }
        if (dx && (r = launch_nhwc_to_nchw(d_dxn, d_dx, B, cin, H, W, cin, 0, c->stream))) return r;
        if (z) {
            if ((r = d_z.alloc(nz))) return r;
            if ((r = launch_nhwc_to_nchw(d_zn, d_z, B, cout, H, W, cout, 0, c->stream))) return r;
        }
        PMX_HIP(hipStreamSynchronize(c->stream));
        if (dx) PMX_HIP(hipMemcpy(dx, d_dx, nx * 4, hipMemcpyDeviceToHost));
        if (dw) PMX_HIP(hipMemcpy(dw, d_dw, ndw * 4, hipMemcpyDeviceToHost));
        if (db) PMX_HIP(hipMemcpy(db, d_db, (size_t)cout * 4, hipMemcpyDeviceToHost));
        if (z) PMX_HIP(hipMemcpy(z, d_z, nz * 4, hipMemcpyDeviceToHost));
        return PMX_OK;
    };
    rc = run();
    if (rc) (void)hipStreamSynchronize(c->stream);        // nothing in flight may outlive the buffers
    return rc;
}

// ---------------------------------------------------------------------------- for pmx_backward.hip
int pmx_run_conv(pmx_ctx* c, const char* label, PackedLayer* L0, PackedLayer* L1, const ConvIO& io, int precision)
{
    FwdCall k = pmx_call(c);
    if (precision >= 0) k.precision = precision;
    return run_conv(c, k, label, L0, L1, io);
}

// The layer whose forward is the data gradient of table layer `layer` (pack_index.h: the transposed pack), packed like any layer, from the
// layer's master weights -- those of the training stores, else the layer's direct pack un-packed into a temporary (the context keeps no
// other copy).  Its input is the layer's g: `cout` channels padded with zeros to 64 for the 38 / 19-channel outputs, so that both branches
// of a launch have the same chunk count.  Its output has the layer's input channels -- for Mconv1_* the 192 channels of the concat buffer
// in the buffer's order, the pad channels zero.
int pmx_bw_transposed_pack(pmx_ctx* c, int layer, bool f16)
{
    PMX_CHECK(layer >= 0 && (size_t)layer < c->layers.size() && (size_t)layer < c->bw.tl.size(), PMX_ERR_INVALID, "backward pack: layer %d", layer);
    PackedLayer& Lt = c->bw.tl[layer];
    // (the f16 pack of the transposed layer: what the dispatcher's f16 form reads, built here so that the chain enqueues without a wait)
    if (Lt.set) return f16 && Lt.ks > 1 ? ensure_f16_pack(c->stream, Lt) : PMX_OK;
    const PackedLayer& L = c->layers[layer];
    PMX_CHECK(L.set, PMX_ERR_WEIGHTS, "backward pack: layer '%s' has no weights", c->table[layer].name.c_str());
    if (L.busy) PMX_HIP(hipStreamSynchronize(L.busy_stream));      // a training step may still be writing d_w and the master weights
    const int kind = pmx_pack_kind(c, L.cin);
    const float* master = pmx_train_master(c, layer);
    DevBuf<float> tmp;
    int rc;
    if (!master) {
        if ((rc = tmp.alloc((size_t)L.cout * L.cin * L.ks * L.ks + L.cout)) || (rc = pmx_unpack_launch(L, kind, tmp, c->stream))) return rc;
        master = tmp;
    }
    PackedLayer P;
    pmx_layer_geometry(P, pmx_pk_t_cout(kind, L.cin), L.cout, L.ks, pmx_pk_t_cin_pad(L.cout));
    if ((rc = build_transposed(P, L.cout, L.cin, L.ks, kind, master, c->stream))) return rc;
    P.set = true; P.busy = L.busy; P.busy_stream = L.busy_stream;
    Lt = std::move(P);
    return f16 && Lt.ks > 1 ? ensure_f16_pack(c->stream, Lt) : PMX_OK;
}
