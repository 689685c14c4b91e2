// pmx_ctx.h -- the context behind the opaque `pmx_ctx*` of the C ABI and the few internal entry points the translation units of the
// ABI share (pmx_api.hip: context, weights, forward plan, post-process, results; pmx_precise.hip: detect_precise and the key-point nets).
#pragma once
#include "pmx_common.h"
#include "pack_index.h"

#include <map>
#include <tuple>
#include <string>
#include <utility>
#include <vector>

// The one owner of a device allocation (Host = true: of pinned host memory).  Every buffer of a context is a member of this type, so
// ~pmx_ctx frees them all and no list of pointers exists anywhere.  `cap` counts elements of T.  Move-only; pointer and capacity always
// travel together.  Converts to T*, so launches and pointer arithmetic read as with a raw pointer.
template <typename T, bool Host = false>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { reset(); swap(o); return *this; }
    ~DevBuf() { reset(); }
    void swap(DevBuf& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
    T* get() const { return p; }
    operator T*() const { return p; }
    size_t capacity() const { return cap; }
    void reset()
    {
        if (p) (void)(Host ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
    // frees what it holds, then allocates exactly `count` elements (16 bytes for none); holds nothing after a failure
    int alloc(size_t count)
    {
        reset();
        const size_t bytes = count * sizeof(T) ? count * sizeof(T) : 16;
        const hipError_t e = Host ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            pmx_set_error("DevBuf: %s of %zu bytes -> %s", Host ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
            return PMX_ERR_HIP;
        }
        cap = count;
        return PMX_OK;
    }
    // grows to `count` elements once `stream` no longer uses the old buffer; a site that needs another synchronisation (or none) calls alloc
    int ensure(size_t count, hipStream_t stream)
    {
        if (count <= cap) return PMX_OK;
        PMX_HIP(hipStreamSynchronize(stream));
        return alloc(count);
    }
};
template <typename T> using HostBuf = DevBuf<T, true>;

static inline size_t pmx_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The one owner of a HIP event.  Empty until create(), which keeps the site's flags (0 = timing enabled); destroyed with its owner.
// Move-only -- a move hands the handle over and calls nothing in HIP; converts to hipEvent_t.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { std::swap(e, o.e); return *this; }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
    int create(unsigned flags)      // no-op when it holds one
    {
        if (!e) PMX_HIP(hipEventCreateWithFlags(&e, flags));
        return PMX_OK;
    }
};

// The one owner of a HIP stream the context created itself (own_stream, lanes 1 .. 3); a caller's stream stays a plain hipStream_t.
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
    int create(unsigned flags, int priority = 0)      // no-op when it holds one
    {
        if (!s) PMX_HIP(hipStreamCreateWithPriority(&s, flags, priority));
        return PMX_OK;
    }
};

// The per-call staging block of a feature: tables built on the host in pinned memory and copied to the device in ONE piece.  The order
// of the steps is the protocol -- the pinned half is not rewritten before the previous copy has read it (`copied`), the device half is
// not reallocated under queued launches (DevBuf::ensure) -- and lives here only.
struct Staging {
    HostBuf<char> host;
    DevBuf<char> dev;
    Event copied;                   // the last copy has left the pinned half
    bool pending = false;           // ... and nobody has waited for it yet
    // both halves at `bytes` at least (grown to exactly that), the pinned one free to be written; the device address is final, so the
    // caller may write it into its tables.  Nothing is pending after a failure.
    int begin(size_t bytes, hipStream_t stream, char** h, char** d)
    {
        if (pending) { pending = false; PMX_HIP(hipEventSynchronize(copied)); }
        int rc;
        if (bytes > host.capacity() && (rc = host.alloc(bytes))) return rc;
        if ((rc = dev.ensure(bytes, stream)) || (rc = copied.create(hipEventDisableTiming))) return rc;
        *h = host; *d = dev;
        return PMX_OK;
    }
    // the first `bytes` bytes -> device, valid for what `stream` runs next
    int commit(size_t bytes, hipStream_t stream)
    {
        PMX_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream));
        PMX_HIP(hipEventRecord(copied, stream));
        pending = true;
        return PMX_OK;
    }
    void reset() { host.reset(); dev.reset(); pending = false; }
};

struct LayerDesc { std::string name; int cin, cout, ks; };

enum NetKind { NET_POSE = 0, NET_FACE = 1, NET_HAND = 2 };     // params['archs'] (entity.py:50-54)

static const int CK = 16;   // channel chunk of every kernel variant

struct PackedLayer {
    bool set = false;
    DevBuf<float> d_w, d_b;
    DevBuf<float> d_ww;          // Winograd F(2x2,3x3) pack [freq 16][chunk32][cout_pad][32] = G g G^T (3x3 layers; option "conv_algo" = 1)
    DevBuf<uint16_t> d_w3;       // bf16x3 pack [tap][chunk][plane hi|mid|lo][cout_pad][16] of d_w (3x3 / 7x7 layers; option "precision" = 1)
    DevBuf<uint16_t> d_w16;      // f16 pack [tap][chunk][cout_pad][16] of d_w (3x3 / 7x7 layers; option "precision" = 2)
    int cin = 0, cout = 0, ks = 0, cin_pad = 0, cout_pad = 0, nch = 0;
    // training (pmx_train.hip): a step rewrites d_w, and every derived pack that exists, in place on `busy_stream` without telling the
    // host, so a lazy builder that derives a pack from d_w on another stream waits for that stream first (busy)
    bool busy = false;
    hipStream_t busy_stream = nullptr;
};

// ------------------------------------------------------------------------------------------ profiler
struct ProfEntry {
    std::string name;
    double total_ms = 0;
    int64_t launches = 0;
    double flops = 0, bytes = 0;   // per launch: algorithmic FLOP of the convolution, compulsory bytes
    double issued = 0;             // per launch: FLOP the kernel issues to the matrix cores for real outputs (Winograd forms: 16/36, 100/196 of
                                   // the algorithmic figure; direct kernels: all of it; tile padding is not counted)
};
struct ProfPending { int entry; Event e0, e1; };

// The working set of one network forward: the padded float input, the activation ping-pong, the concat buffer and the branch buffers, the
// uint8 network input, detect_precise's up-sampled maps of one scale (planar [n][38][ph][pw] | [n][19][ph][pw]) and the partial-sum
// slabs of the split-K / unit-mode launches.  The context is one (its own: every forward that does not run on a lane, and what the
// post-process, the loss, the backward and the box code mean by c->cat, c->act1, ...); every lane of detect_precise holds another.
struct NetBufs {
    DevBuf<float> in16, act0, act1, cat, brA, brB, brT;
    DevBuf<uint8_t> u8_tmp;
    DevBuf<float> pr_tmp, sk_scratch;
};

// detect_precise runs its inference scales CONCURRENTLY: one image at 0.5x / 1x / 1.5x is 12 ... 108 one-per-CU blocks per layer for 256
// CUs, so the four forward passes go to four streams ("lanes"), each with its own working set; the forward of a scale is handed its
// lane's set and stream in its FwdCall, the context's own stay what they are.  The first scale enqueued in a
// sequence runs on lane 3 (highest stream priority), the others round-robin on the remaining lanes in use (pmx_precise.hip); the scale in
// slot k leaves its maps, resized to the original size, in pr_part[k]; pmx_precise_finish adds the parts IN SLOT ORDER
// (the reference's left-to-right sum, pose_detector.py:463,467) and divides.
constexpr int PMX_PR_LANES = 4;
constexpr int PMX_SK_ZERO_BIAS = 1024;      // floats of the shared zero-bias vector of the split-K / unit-mode launches
struct PrLane {
    Stream stream;                           // lanes 1 .. 3 (lane 0 runs on the context's stream, in the context's own set)
    Event done;
    NetBufs ws;
    size_t cap_px = 0;                       // n * padded_h * padded_w the activation buffers hold
};

// Heterogeneous batches (pmx_multi.hip): a SEGMENT = n images of one network-input size.  The segments of a forward lie end to end in
// every activation buffer; per resolution level (0 = input .. 3 = 1/8) and tile shape a device table tells the kernels which tiles
// belong to which segment (pmx_common.h::ConvSeg).  Tables of one forward: conv1's 16 x 16 squares at level 0 (output = level 1), the
// 8 x 16 rectangles of levels 1, 2 (un-pooled / pooled output) and 3.
struct SegDesc { int n, H, W; };
// f16 mode (option "precision" = 2) runs conv1_1 / conv1_2 on 8 x 16 rectangles of level 0 as well: tables L0 (output at level 0) and L0P
// (pooled: output at level 1).
enum { PMX_SEG_CONV1 = 0, PMX_SEG_L1 = 1, PMX_SEG_L1P = 2, PMX_SEG_L2 = 3, PMX_SEG_L2P = 4, PMX_SEG_L3 = 5, PMX_SEG_L0 = 6, PMX_SEG_L0P = 7,
       PMX_SEG_TABLES = 8 };
#define PMX_SEG_RECT(level, pool) ((level) == 0 ? ((pool) ? PMX_SEG_L0P : PMX_SEG_L0) : (level) == 1 ? ((pool) ? PMX_SEG_L1P : PMX_SEG_L1) \
                                   : (level) == 2 ? ((pool) ? PMX_SEG_L2P : PMX_SEG_L2) : PMX_SEG_L3)
// the host description of one segment: n images of network input H x W (mh x mw: the up-sampled map size of pmx_detect_images, else 0)
struct SegGeo { int n, H, W, mh, mw; };
// the segment tables of ONE heterogeneous forward (build_seg_tables): the segments, tiles per launch per table, pixels of all segments per
// level, and the device tables -- PMX_SEG_TABLES tables of segs.size() entries in c->d_segs, valid until the next build
struct SegTables {
    std::vector<SegDesc> segs;
    int tiles[PMX_SEG_TABLES] = {};
    long long pix[4] = {};
    const ConvSeg* dev = nullptr;
    const ConvSeg* table(int t) const { return dev + (size_t)t * segs.size(); }
};
// What one network forward runs on and over, handed from its entry down to every launch by const reference: nothing a forward needs to
// know about its own call is a member of the context.  pmx_call(c) is the call of everything that runs on the context itself.
// Two half-batch chains (option "batch_chains"; pmx_detect_batch): the images [0, n0) of a uniform batch run on the call's stream, the images
// [n0, B) on the context's second stream, with every buffer that is indexed by image shared at the image offset and a scratch of its own
// for what is not (the slabs of the split-K / unit-mode / tail launches and their zero bias).  Every layer is planned ONCE for the whole
// batch and the plan launched per chain -- layer i of chain 0, then layer i of chain 1 -- so an image's arithmetic is that of the one-chain
// form.  `probe`: nothing is launched; the forward only finds out whether every layer keeps its whole-batch plan on a half (ok) and whether
// the halves of every 7x7 plain launch are whole rounds of the CUs (rounds: the automatic rule, conv_select.hip::batch_chains_rounds).
struct BatchChain {
    Stream stream;
    Event fork, done;
    DevBuf<float> sk_scratch, sk_zero_bias;
};
struct ChainSplit {
    int n0 = 0;                      // images of the first chain
    size_t net_px = 0;               // pixels of one network input (what places the second chain in act0 / act1: pmx_api.hip, image_offset)
    BatchChain* second = nullptr;
    bool probe = false, ok = true, rounds = true;
};
struct FwdCall {
    NetBufs& ws;                     // the working set: the context's own or a lane's
    hipStream_t stream;              // what every launch and profile event of the forward is enqueued on
    int conv_algo;                   // option "conv_algo" for this forward
    int precision;                   // option "precision" for this forward (a data gradient of pmx_conv2d_backward or of the head chain under
                                     // "grad_precision" 2: 2)
    const SegTables* seg = nullptr;  // a heterogeneous forward: its tables (null: a uniform batch)
    const uint8_t* in_u8 = nullptr;  // conv1_wino_kernel preprocesses this uint8 batch itself (null: the float input in ws.in16)
    float in_div = 255.0f;           // ... dividing by this
    ChainSplit* split = nullptr;     // the forward runs as two half-batch chains (null: one chain)
    BatchChain* scratch = nullptr;   // the launches of the second chain: its slabs and zero bias (null: ws.sk_scratch, the context's zero bias)
};
// The channel slices of one NHWC buffer that the (up to two) groups of a launch read or write, `ld` floats per pixel.  one: a single group;
// two: both branches side by side in the buffer, the second `off` channels after the first (the pose network's brA / brB / brT / cat).
struct ConvBuf {
    float* p[2];
    int ld;
    static ConvBuf one(float* p, int ld) { return {{p, nullptr}, ld}; }
    static ConvBuf two(float* p, int off, int ld) { return {{p, p + off}, ld}; }
};
// What a caller says about one layer launch: where its groups read and write (pointers already at the group's channels, [1] null: one
// group), the batch, the INPUT map size and what follows the convolution.  `level` (heterogeneous forward only, FwdCall::seg set): the
// resolution level of the layer's input, 0 = network input .. 3 = 1/8; B, H, W then carry the image count and the LARGEST map of the
// level (launch checks), the geometry comes from the segment table of the level.
struct ConvIO {
    const float* in[2]; int lda;
    float* out[2]; int ldc;
    int B, H, W, relu, pool, level;
};
static inline ConvIO conv_io(const ConvBuf& in, const ConvBuf& out, int B, int H, int W, int relu, int pool, int level = -1)
{
    return {{in.p[0], in.p[1]}, in.ld, {out.p[0], out.p[1]}, out.ld, B, H, W, relu, pool, level};
}
// one post-process launch set of the current results: a uniform batch is one call (base 0), a mixed batch one per segment
struct PPCall { PPMaps maps; PPTables tab; int base, B, map_h, map_w; double img_len; bool has_scale; int limbs_slices; };

// Head backward (pmx_backward.hip; include/pose_mi355x.h: pmx_backward_head).  The 82 layers after conv4_2 share 42 SLOTS of one layout,
// used twice: `act` (the retained outputs a) and `g` (the masked gradients).  A slot holds both branches of a layer pair side by side,
// [pixel][L1 | L2], as the forward's brA / brB / brT do, so a retaining forward writes its outputs straight into `act`.
//   PMX_BW_C43       conv4_3_CPM, 256 floats per pixel            PMX_BW_C44  conv4_4_CPM: g only (128); a = channels 0 .. 127 of c->cat
//   PMX_BW_S1 + i    conv5_{i+1}_CPM, i = 0 .. 2: 2 x 128; i = 3: 2 x 512; i = 4 (conv5_5_CPM): a stage output
//   PMX_BW_M(s, i)   Mconv{i}_stage{s}: i = 1 .. 6: 2 x 128; i = 7: a stage output
//   PMX_BW_X42       conv4_2's output, 512 (a only)
// stage output: a = [38 PAF, 2 zeros | 19 heat, 5 zeros] (channels 128 .. 191 of c->cat, copied after the stage's loss launch); g =
// [38 PAF, zeros to 64 | 19 heat, zeros to 128] (every branch's g starts at a multiple of 32 floats and is zero-padded to one)
enum { PMX_BW_C43 = 0, PMX_BW_C44 = 1, PMX_BW_S1 = 2, PMX_BW_M2 = 7, PMX_BW_X42 = 42, PMX_BW_SLOTS = 43 };
#define PMX_BW_M(s, i) (PMX_BW_M2 + ((s) - 2) * 7 + (i) - 1)
struct BwSlot { size_t a_off = 0, g_off = 0; int lda = 0, ldg = 0; };
struct BwState {
    int on = 0;                                           // pmx_backward_enable: 0 off, 1 the head, 2 the head and the trunk
    bool valid = false;                                   // the last forward retained (cleared by every other forward)
    bool done = false;                                    // pmx_backward_head ran for it
    int stages = 0, B = 0, fh = 0, fw = 0;                // ... its stages and shape
    size_t cap_px = 0;                                    // pixels (images x h/8 x w/8) the stores hold
    BwSlot slot[PMX_BW_SLOTS];
    DevBuf<float> act, g;                                 // the two stores
    DevBuf<float> grad;                                   // dw (OIHW) | db of every layer: grad_off[layer], then cout * cin * ks^2 floats further
    std::vector<size_t> grad_off;                         // by index into c->table (trunk layers: mode 2 only, after every head layer's)
    DevBuf<float> u;                                      // dx of the layer just run = the upstream gradient of the one before: [pixel][<= 1024]
    DevBuf<float> dcat;                                   // dx of Mconv1_stage{s}_L1 | _L2 in concat-buffer order: [pixel][2 x 192]
    DevBuf<float> fg;                                     // the running sum at the feature map: [pixel][128]
    DevBuf<float> trunk;                                  // dx of conv4_3_CPM: [pixel][512]
    DevBuf<float> ws;                                     // weight-gradient workspace (grown before a backward is enqueued)
    DevBuf<double> part;                                  // bias-gradient slots
    DevBuf<int> cat_of_ref;                               // concat-buffer channel of the reference's input channel 0 .. 184 of Mconv1_*
    std::vector<PackedLayer> tl;                          // per layer: the pack whose forward is the data gradient (set = built)
    bool stepped = false;                                 // pmx_train_step_head or pmx_train_step consumed the gradients of this backward
    int slot_layer[PMX_BW_SLOTS][2] = {};                 // table index of the slot's L1 / L2 layer (one-branch slots: both the same; X42: conv4_2)
    std::vector<int> layer_slot;                          // by table index: slot * 2 + branch, -1 for the trunk layers before conv4_2
    // Trunk backward (mode 2; include/pose_mi355x.h: pmx_backward_trunk).  The ten layers conv1_1 .. conv4_2 in forward order, t = 0 .. 9, at
    // resolution level 0, 0, 1, 1, 2, 2, 2, 2, 3, 3 (level l: h / 2^l x w / 2^l).  `t_act` holds, NHWC with the layer's own channel count per
    // pixel: the post-ReLU, PRE-pool output a of t = 0 .. 8 at t_a_off[t] (conv4_2's is slot PMX_BW_X42) and the pooled maps of conv1_2,
    // conv2_2, conv3_4 at t_p_off[0 .. 2].  One pair of gradient buffers serves the whole chain, each as large as the widest layer (64
    // floats per input pixel): t_g = the masked gradient g of the layer being run, t_u = its dx, the upstream gradient of the layer before.
    // t_gk (option "trunk_keep_g" at enable time; tests): a g slot per layer at t_g_off[t] instead of the shared t_g, for pmx_get_retained.
    bool trunk_done = false;                              // pmx_backward_trunk ran for the retained forward
    int t_H = 0, t_W = 0;                                 // the retained forward's network-input size
    int t_layer[10] = {};                                 // table index of trunk layer t
    size_t t_a_off[10] = {}, t_p_off[3] = {}, t_g_off[10] = {};
    DevBuf<float> t_act, t_u, t_g, t_gk;
};
constexpr int PMX_TRUNK_LAYERS = 10;
struct TrunkDesc { const char* name; int cin, cout, level, pool; };      // pool: the forward pools this layer's output
extern const TrunkDesc pmx_trunk_desc[PMX_TRUNK_LAYERS];

// Training steps (pmx_train.hip; include/pose_mi355x.h: pmx_train_*).  Three stores with the layout of BwState::grad -- per head layer, in
// mode 2 per trunk layer as well, w | b at grad_off[layer], padded to a multiple of 64 floats: the master weights (OIHW, reference input
// order), Adam's first and second moments.  Per layer of c->table: its step count and gradient scale (trunk layers: used in mode 2).
// seg: the tables of one step -- the Adam segments, then the packers' jobs (pmx_train.hip: jobs_at).
struct AdamSeg { unsigned long long off; unsigned n, blk0; float scale, alpha_t; };      // blk0: first block of the segment in the launch
struct TrainState {
    int on = 0;
    DevBuf<float> w, m, v;
    std::vector<int> t;
    std::vector<float> scale;
    double alpha = 1e-4, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
    Staging seg;
};

// ------------------------------------------------------------------------------------------- context
struct pmx_ctx : NetBufs {           // (the base: the context's own working set)
    // heterogeneous forward / post-process state.  Whether a forward is heterogeneous is a property of its FwdCall (seg), not of the context
    std::vector<SegDesc> cur_segs;   // layout of the current network output when it came from a heterogeneous forward (else empty)
    DevBuf<ConvSeg> d_segs;                               // device: the tables of the last build_seg_tables (SegTables::dev points here)
    std::vector<PPCall> pp_calls;                         // non-empty: the post-process of the current results ran per segment
    // table sets per (in_h, in_w, out_h, out_w) of the per-segment calls: the kernel-argument struct and the one allocation [grid | taps] it points into
    std::map<std::tuple<int, int, int, int>, std::pair<PPTables, DevBuf<char>>> tab_cache;
    DevBuf<uint8_t> mi_src;                               // pmx_detect_images: original-size images awaiting the device resize
    DevBuf<int> mi_tab;                                   // ... and their resize tables
    // pmx_detect_precise_images (pmx_precise_images.hip): per-call buffers, grown on demand and never keyed by size.  pi_dev holds the
    // call's descriptors, cubic tables and post-process tables (ONE upload); it stays untouched until the next call, so a grow-and-re-run
    // of the post-process (pp_calls) still finds its tables there.
    DevBuf<char> pi_dev;
    DevBuf<uint8_t> pi_src;                               // the original images, end to end
    DevBuf<float> pi_tmp;                                 // x8 up-sampled maps per (image, scale) pair, planar [57][ph][pw]
    DevBuf<float> pi_maps;                                // averaged full-resolution maps per image, planar [38 PAF | 19 heat][orig_h][orig_w]
    std::vector<long long> pi_off;                        // first float of image i's maps in pi_maps
    std::vector<int> pi_hw;                               // (orig_h, orig_w) of image i
    int kind = NET_POSE;             // architecture: posenet | facenet | handnet
    int n_heat = PMX_N_HEAT;         // heat-map channels of the last layer (19 | 71 | 22)
    int cat_c = PMX_CAT_C;           // channels of the cat buffer (192 | 208 | 160)
    int cat_heat = PMX_CAT_HEAT;     // first heat-map channel in the cat buffer (168 | 128 | 128)
    // detect_precise accumulation state (pmx_precise_*)
    int pr_h = 0, pr_w = 0, pr_scales = 0, pr_n = 0;      // original size, scales accumulated so far, images of the batch
    unsigned pr_mask = 0;                                 // slots (positions in the reference's scale loop) filled so far
    std::map<std::tuple<int, int, int>, DevBuf<int>> pr_tabs; // cubic tables per axis, keyed (src, dst, fixed point?): built once, kept
    const uint8_t* pr_src = nullptr;                     // host images of the current begin / finish sequence already in u8_src
    PrLane pr_lane[PMX_PR_LANES];                        // lanes 1 .. : own streams and sets; lane 0 = the context's own (its ws stays empty)
    std::vector<DevBuf<float>> pr_part;                  // per scale: [n][57][orig_h][orig_w] (PAF planes, then heat planes of every image)
    Event pr_src_ready, pr_fin;                          // originals uploaded / parts consumed by the last finish
    int opt_precise_lanes = PMX_PR_LANES;                // 1: every scale on the context's own stream (A/B, tests)
    int opt_precise_plain = -1;                          // detect_precise's forwards on the plain Winograd kernels: -1 = when all four lanes are in use, 0 never, 1 always
    int opt_precise_lane_priority = 1;                   // lane streams with priorities (largest scale first); read when a lane's stream is created
    int opt_precise_table_cap = 208;                     // cached cubic tables at which the next pmx_precise_begin* starts the cache over (256 - 48)
    int pr_tabs_trims = 0;                               // how often that happened (diagnostics: option query "precise_table_trims")
    DevBuf<double> d_kp;             // key-point records of pmx_keypoints
    int device = 0;
    int num_cus = 256;               // compute units of `device` (pmx_create_net): what kernel / tile selection counts blocks against
    hipStream_t stream = nullptr;    // what everything is enqueued on: own_stream or the caller's (pmx_set_stream), never destroyed here
    Stream own_stream;
    int max_batch = 0, max_h = 0, max_w = 0;
    std::vector<LayerDesc> table;
    std::map<std::string, int> index;
    std::vector<PackedLayer> layers;
    // buffers (besides the working set)
    DevBuf<float> nchw_tmp;          // staging for NCHW host <-> NHWC device conversions
    DevBuf<uint8_t> u8_src;         // original-size images awaiting the on-device resize
    DevBuf<int> rs_tab;              // resize tables: x (4 * dw ints) then y (4 * dh ints)
    int rs_key[4] = {0, 0, 0, 0};    // (src_h, src_w, h, w) of the tables rs_tab holds; all 0: none
    // state of the last forward / set_maps
    bool maps_valid = false, maps_external = false;
    int cur_B = 0, cur_fh = 0, cur_fw = 0;
    DevBuf<float> ext_paf, ext_heat;                 // NCHW copies installed by pmx_set_maps
    // post-process
    PPTables tab{};                  // kernel arguments: raw pointers into tab_store (pmx_ensure_tables)
    DevBuf<char> tab_store;          // [grid of (tab_out_h, tab_out_w) | taps] (pp_tables.h)
    int tab_in_h = -1, tab_in_w = -1, tab_out_h = -1, tab_out_w = -1;
    std::vector<double> gauss;
    PPBuffers pp{};                  // kernel arguments: raw pointers into pp_store (pp_alloc) and, pp.smoothed, to `smoothed`
    DevBuf<char> pp_store;
    DevBuf<float> smoothed;          // optional smoothed maps, sized on demand (pmx_ensure_smoothed)
    DevBuf<double> d_scale;
    HostBuf<unsigned char> h_results;           // pinned staging for pmx_get_results (pageable D2H is slow and jittery)
    // pmx_results_snapshot / pmx_snapshot_wait: PMX_SNAPSHOT_SLOTS slots (event, pinned status words, layout at snapshot time)
    Event snap_ev[PMX_SNAPSHOT_SLOTS];
    HostBuf<int> snap_status[PMX_SNAPSHOT_SLOTS];
    int snap_B[PMX_SNAPSHOT_SLOTS] = {}, snap_cap_ppl[PMX_SNAPSHOT_SLOTS] = {};
    size_t snap_rec[PMX_SNAPSHOT_SLOTS] = {};
    bool pp_valid = false;
    bool pp_final = false;                      // statuses checked: no image of the last post-process overflowed a capacity
    int pp_B = 0, pp_h = 0, pp_w = 0;
    // arguments of the last post-process, kept for the grow-and-re-run
    PPMaps pp_maps{};
    double pp_img_len = 0;
    bool pp_has_scale = false;
    int pp_regrown = 0;                         // number of capacity growths so far (diagnostics)
    // options
    int opt_force[8] = {-1, -1, -1, -1, -1, -1, -1, -1};   // by ksize
    int opt_gpu_branch_peaks = 0;    // reference GPU-branch peak extraction (non-golden variant)
    int opt_limbs_slices = -1;       // blocks per (limb, image) of the candidate scan: -1 = 8 for full-resolution (external) maps, else one; same results
    int pp_limbs_slices = 0;         // ... of the last post-process (kept for the grow-and-re-run)
    int opt_kp_flip_x = 0;           // pmx_keypoints: mirror the resized heat maps left-right before the peaks (hand_detector.py:46-47)
    int tab_flip = 0;
    int opt_keep_smoothed = 0, opt_stop_stage = 6, opt_kernel_gen = 6;
    int opt_conv_algo = 1;           // 1 (default): Winograd F(2x2,3x3) fp32 kernel for the 3x3 / 7x7 layers of launches that fill the chip
                                     // (>= 2 blocks per CU: batches); 0: direct kernels everywhere; 2: Winograd on every eligible layer
                                     // (tests).  Both are fp32 with a defined order and a C twin; they differ by fp32 rounding (~1e-6)
    int opt_wino_unit_eff = 80;      // unit mode: in-round efficiency of the 7x7 unit blocks relative to the plain kernel, percent (cost model;
                                     // measured with tools/wino_batch_sweep.py: 75 - 90 alike, 60 loses batch 4 and 8, 105 loses batch 16+)
    int opt_wino_min_fill = 50;      // conv_algo 1: percent of ceil(blocks / CUs) * CUs block slots a launch must fill to take the Winograd kernel
    int opt_wino_geom = -1;          // Winograd block geometry on 46-pixel-wide maps: -1 / 1 runs of 32 consecutive tiles, 0 the 8 x 16 pixel rectangles
                                     // of every other map size (same bits either way)
    int opt_wino_tail = -1;          // run geometry: the part-filled last block of every image in unit mode (K units + combine) -- -1 by the cost
                                     // model (conv_algo 1), 0 never, 1 wherever a unit plan exists.  Changes the summation of those tiles (C twin: unit_from)
    int opt_wino_tail_merge = 1;     // the tails of all images of a launch as one stream of tiles, 32 per block (0: one part-filled block per image)
    int opt_wino_tail_g = 0;         // tuning: chunks per pass-1 unit of the tail (0 = automatic)
    int opt_wino_split = 1;          // a batch whose plain launch ends in a part-filled round of the CUs is cut in two by images (0: never)
    int opt_batch_chains = -1;       // pmx_detect_batch on a uniform fp32 batch as two half-batch chains on two streams (BatchChain): 0 never, 1 wherever
                                     // every layer keeps its whole-batch plan on a half, -1 (default) by the rule of conv_select.hip::batch_chains_rounds
    BatchChain chain2;               // the second chain: stream, events and scratch, made on first use
    int chains_key[4] = {0, 0, 0, -1};   // (B, H, W, opt_epoch) of the last probe, chains_ok / chains_rounds its verdict
    bool chains_ok = false, chains_rounds = false;
    int opt_epoch = 0;               // counts pmx_set_option calls: what was decided from the options is decided again
    int opt_wino_unit_g = 0;         // tuning: chunks per pass-1 unit of a launch in unit mode (0 = automatic, -1 = as many units as 8 slabs allow)
    int opt_precision = 0;           // 0: fp32 MFMA everywhere (the path whose results are specified); 1: bf16x3 kernels where a
                                     // v6 kernel would run (fp32-grade accuracy at 2.67x the matrix rate, NOT the fp32 FMA chain);
                                     // 2: f16 mode -- every 3x3 / 7x7 layer on conv_f16_kernel (f16 operands, fp32 sums; the 1x1 layers stay fp32)
    int opt_f16_bn = 0;              // f16 mode: output channels per block, 0 = conv_f16_bn's rule, 64 | 128 = that width (same bits; tests)
    int opt_conv1_wino = 1;          // fused conv1_1 + conv1_2 with conv1_2 as Winograd F(2x2, 3x3) (conv1_wino_kernel) where conv_algo allows Winograd
    int opt_fuse_conv1 = 1;          // conv1_1 recomputed on conv1_2's halo tile, one launch (conv1_fused_kernel); identical bits
    int opt_fuse_pairs = 1;          // the two 1x1 layers that end every stage run as one launch (conv1x1_pair_kernel)
    int opt_ksplit = 0;              // 0: automatic split-K for small launches; n > 0: force n K slices where split-K applies
    // kernel-form switches for tests and tuning: either setting computes the same bits
    int opt_conv_min_lds = 0;        // dynamic LDS floor of every direct kernel: caps the co-resident blocks per CU (the fp32 MFMA
                                     // pipe loses ~20% with 3+ waves per SIMD)
    int opt_conv_v5_lds = 56 * 1024; // ... of the v5 / v8 kernels: 3 x 56 KB > 160 KB -> at most 2 blocks per CU
    int opt_pp_generic = 0;          // 1: always the generic-radius peaks kernel
    int opt_cubic_rows = 1;          // detect_precise's cubic resize: 1 the separable form through LDS, 0 one thread per element
    // split-K: the zero bias vector of the slice blocks, shared by every working set (each has its own slabs, sk_scratch)
    DevBuf<float> sk_zero_bias;
    // timing / profiling
    Event t0, t1;
    int prof_on = 0;                 // 0 off | 1 every launch | 2 only the 7x7 convolutions (the dominant kernel: fewest events in a timed region)
    std::vector<ProfEntry> prof;
    std::map<std::string, int> prof_index;
    std::vector<ProfPending> pending;
    std::vector<Event> ev_pool;        // recycled events (creating two per launch inside the timed region costs ~0.5 %)
    int prof_open = -1;
    // pmx_boxes.hip (key points for many boxes of one image).  bx: [resize tables | crop / tile tables | up-sampling grids]; bx_rec: the
    // per-tile arg-max records of the key points.
    Staging bx;
    DevBuf<char> bx_rec;
    // pmx_loss.hip (validation loss).  Targets at h/8 x w/8, [image][map pixel][38 PAF | 19 heat] (the cat slices' order), the resized ignore
    // mask [image][map pixel]; the poses they came from (device: label kernel; host: pmx_get_labels); the corner-aligned grid of (h, w) ->
    // (h/8, w/8); per (stage slot, block, branch) partial sums and the 2 x PMX_LOSS_SLOTS means.  Slot PMX_LOSS_SLOTS - 1 = pmx_loss_current_maps.
    DevBuf<float> ls_tgt, ls_full;                        // ls_full: 57 full-resolution planes of ONE image (pmx_get_labels, pmx_loss_set_targets)
    DevBuf<uint8_t> ls_mask, ls_mask_in;
    DevBuf<double> ls_poses, ls_part, ls_out;
    DevBuf<int> ls_off;                                   // first person of image b (batch + 1 entries)
    DevBuf<char> ls_grid;                                 // the grid block of (h, w) -> (h/8, w/8) (pp_tables.h), ls_tab its pointers
    PPTables ls_tab{};
    std::vector<double> ls_h_poses; std::vector<int> ls_h_off;
    std::vector<uint8_t> ls_h_mask;                       // the caller's ignore mask, copied before the call returns (the upload reads this copy)
    double ls_sigma = 0, ls_width = 0;
    int ls_grid_h = 0, ls_grid_w = 0;
    int ls_on = 0;                                        // pmx_loss_enable
    int ls_B = 0, ls_h = 0, ls_w = 0;                     // the targets' batch and network-input size (0: no targets)
    bool ls_have_poses = false;
    int ls_stages = 0;                                    // stages of the last hooked forward (0: none yet)
    // pmx_loss_grad_enable: d(total_loss)/dy of every stage, [stage][image][map pixel][38 PAF | 19 heat], allocated when first switched on
    DevBuf<float> ls_grad;
    int lg_on = 0;
    int lg_stages = 0, lg_B = 0, lg_fh = 0, lg_fw = 0;    // the hooked forward whose gradients ls_grad holds (lg_stages 0: none)
    int lg_scale_log2 = 0;                                // ... and the "loss_scale_log2" it ran under: ls_grad holds 2^k times the gradients
    int opt_loss_scale_log2 = 0;                          // k = 0 .. 24: the next hooked forward hands loss_grad_kernel its two constants times 2^k
    // pmx_conv2d_backward: test-only, S0 of the weight-gradient strips (0: automatic); include/pose_mi355x.h
    int opt_wgrad_strips = 0;
    // pmx_conv2d_backward and pmx_backward_head: 0 fp32 gradients; 2: dw and dx of a 3x3 / 7x7 layer with f16 operands and fp32 sums
    // (include/pose_mi355x.h)
    int opt_grad_precision = 0;
    int opt_trunk_keep_g = 0;        // read by pmx_backward_enable(2): keep the masked gradient of every trunk layer for pmx_get_retained (tests)
    // pmx_samples.hip (sample preparation).  sp: [descriptors | resize tables | host sources]; sp_a: the resized intermediates of the
    // training samples; sp_out: max_batch x insize x insize x 3 prepared images; sp_mask_raw / sp_mask_tmp / sp_mask: the mask before, between
    // and after the two dilation passes; sp_const: the weight and division tables of the contract (uploaded once).
    Staging sp;
    DevBuf<char> sp_const;
    DevBuf<uint8_t> sp_a, sp_out, sp_mask_raw, sp_mask_tmp, sp_mask;
    int sp_n = 0, sp_insize = 0;                          // the prepared samples (0: none)
    // pmx_render.hip (result images).  rd: [image table | primitives]; rd_img: the host images of the call; rd_out: the canvases end to
    // end when the caller's output is host memory.  All grow on demand (original images are larger than the network input).
    Staging rd;
    DevBuf<uint8_t> rd_img, rd_out;
    // pmx_masks.hip (ignore masks).  mk: [image table | parts | vertices | running sums]; mk_out: the masks end to end when the caller's
    // output is host memory.  All grow on demand.
    Staging mk;
    DevBuf<uint8_t> mk_out;
    // pmx_eval.hip (COCO key-point evaluation).  ev: [image table | ground truths | constants | scores | poses]; ev_out: every output
    // table of the call.  Both grow on demand.
    Staging ev;
    DevBuf<char> ev_out;
    BwState bw;                                          // pmx_backward.hip
    TrainState tr;                                        // pmx_train.hip
};
constexpr int PMX_LOSS_SLOTS = 7;
constexpr int PMX_LOSS_MAX_BLOCKS = 256;

#define PMX_DEV(c) PMX_HIP(hipSetDevice((c)->device))
// the default call of a context: its own working set, its stream, its "conv_algo" and "precision"
static inline FwdCall pmx_call(pmx_ctx* c) { return FwdCall{*c, c->stream, c->opt_conv_algo, c->opt_precision}; }

// pmx_api.hip
// the network on a uint8 BGR batch on the device: preprocess (x / divisor - 0.5) + forward; where conv1 runs as conv1_wino_kernel the
// preprocessing happens inside it (no float copy of the input), else prep_u8 fills k.ws.in16 first
int pmx_forward_from_u8(pmx_ctx* c, const FwdCall& k, const uint8_t* d_u8, int B, int H, int W, float divisor);
int pmx_forward_from_in16(pmx_ctx* c, const FwdCall& k, int B, int H, int W);      // the network on the padded float input already in k.ws.in16
// up-sampling tables of the post-process.  On any failure the context stays consistent: c->tab points into whatever c->tab_store holds (or
// nowhere) and tab_in_h is invalid, so the next call rebuilds
int pmx_ensure_tables(pmx_ctx* c, int in_h, int in_w, int out_h, int out_w, int flip_x = 0);
PPBuffers pmx_pp_view(const PPBuffers& p, int base);         // the post-process buffers of the images [base, ...) (every per-image array offset)
void pmx_make_resize_table(int dst, int src, int* tab);      // OpenCV INTER_LINEAR uint8 table of one axis: [idx0 | idx1 | coef0 | coef1] x dst
int pmx_check_weights(pmx_ctx* c);                          // PMX_ERR_WEIGHTS unless every layer has weights
int pmx_prof_begin(pmx_ctx* c, const char* name, double bytes);   // per-launch profiler (option 1 only) around one launch
int pmx_prof_end(pmx_ctx* c);
// the taps block of the context's post-process tables (pp_tables.h::pp_taps_build) -> host; t.gauss -> dev, and t's radius, border and
// NMS flags: pmx_set_gaussian's taps with the reflected border and the strict NMS, or the reference's GPU peak branch
void pmx_pp_gauss(const pmx_ctx* c, void* host, void* dev, PPTables& t);
// the current network output of a uniform batch as the post-process reads it: the NCHW copies of pmx_set_maps / pmx_precise_finish or the
// NHWC cat slices of the last stage; the PAF fields only on a posenet context
PPMaps pmx_current_maps(const pmx_ctx* c);
// pmx_precise.hip: the cubic table of one axis for (src -> dst), 8 * dst ints [4 x dst indices | 4 x dst coefficients: float32 bits, or
// OpenCV's 11-bit fixed point for the uint8 resize when `fixed`]
void pmx_cubic_table(int src, int dst, bool fixed, int* out);
// pmx_multi.hip: the segment tables of a forward -> device (synchronises the stream once), and the network over the segments whose uint8
// pixels lie end to end at d_u8 (on the device)
int build_seg_tables(pmx_ctx* c, const std::vector<SegGeo>& g, SegTables& t);
int forward_segments(pmx_ctx* c, const uint8_t* d_u8, const std::vector<SegGeo>& g, int B);
// pmx_loss.hip: the hook of the uniform forward.  pmx_loss_check runs with the forward's argument checks (hook on: targets of this batch and
// size, else PMX_ERR_STATE); pmx_loss_stage enqueues the loss launch of stage `stage` (1 .. 6) over the cat slices, pmx_loss_finish the
// final launch.  PMX_LOSS_NO_MIXED: the refusal of the mixed-size and precise entries while the hook is on.
int pmx_loss_check(pmx_ctx* c, int B, int H, int W);
int pmx_loss_stage(pmx_ctx* c, int stage, int B, int fh, int fw);
int pmx_loss_finish(pmx_ctx* c, int n_stages, int B, int fh, int fw);
// pmx_loss_set_poses with the ignore mask either on the host (copied before return) or already on the device (read where it lies)
int pmx_loss_set_poses_masked(pmx_ctx* c, const double* poses, const int* n_people, int batch, int h, int w, const uint8_t* ignore_mask,
                              bool mask_on_device, double heat_sigma, double paf_width);
#define PMX_LOSS_NO_MIXED(c, what) \
    PMX_CHECK(!(c)->ls_on, PMX_ERR_STATE, what ": the validation-loss hook is on (pmx_loss_enable) and covers uniform batches only")
// conv_bwd.hip: the launches of pmx_conv2d_backward besides the dispatcher's (the entry itself is in pmx_api.hip, next to pmx_conv2d).
// g and x are NHWC with cg = round_up(cout, 32) and cx = round_up(cin, 32) channels per pixel, the padding channels zero.
//   mask   g from dy (NCHW, pooled size if pool) and z (NHWC, ldz floats per pixel): include/pose_mi355x.h; writes all cg channels
//   db     part: slots x cg doubles of workspace; db[co] = (float)(the slots added in slot order)
//   wgrad  strips of `rows` image rows each (`strips` of them cover B * H rows); ws: strips x ks^2 x cg x cx floats; dw OIHW
constexpr int PMX_DB_SLOTS = 64;
int conv_bwd_mask_launch(const float* dy_nchw, const float* z_nhwc, int ldz, float* g, int B, int H, int W, int cout, int cg, int relu, int pool,
                         hipStream_t stream);
// (ldg / ldx: floats per pixel of g / x, >= cg / cx -- the operands may be slices of wider buffers; cin_map, device memory or null: the
// channel of x that holds input channel ci of dw; max_strips: the largest strip count the caller's rule can give)
int conv_bwd_db_launch(const float* g, int ldg, double* part, float* db, long long npix, int cout, int cg, hipStream_t stream);
int conv_wgrad_launch(const float* g, int ldg, const float* x, int ldx, float* ws, float* dw, int B, int H, int W, int cout, int cg, int cin, int cx,
                      int ks, int strips, int rows, const int* cin_map, hipStream_t stream, int max_strips = PMX_WGRAD_MAX_STRIPS);
int conv_wgrad_strips(int B, int H, int cg, int cx, int ks, int forced, int* rows);      // S and, in *rows, R of the header's rule
// the combine of both weight-gradient kernels: dw (OIHW) = the strips' slots [strip][tap][cg][cx] of ws added left to right
int conv_wgrad_combine_launch(const float* ws, float* dw, int strips, int ks, int cout, int cin, int cg, int cx, const int* cin_map, hipStream_t stream);
// conv_wgrad_f16.hip: the weight gradient of a 3x3 / 7x7 layer with f16 operands (option "grad_precision" = 2): conv_wgrad_launch's arguments
// and workspace, ldg / ldx multiples of 4 and g / x 16-byte aligned; (strips, rows) from conv_wgrad_f16_strips
int conv_wgrad_f16_launch(const float* g, int ldg, const float* x, int ldx, float* ws, float* dw, int B, int H, int W, int cout, int cg, int cin, int cx,
                          int ks, int strips, int rows, const int* cin_map, hipStream_t stream, int max_strips = PMX_WGRAD_MAX_STRIPS);
int conv_wgrad_f16_strips(int B, int H, int cg, int cx, int ks, int forced, int* rows);
int conv_wgrad_trunk_strips(int B, int H, int cg, int cx, int forced, int* rows);        // ... of the trunk chain's rule (3x3 layers)
// conv_bwd.hip: the trunk backward's own launches (include/pose_mi355x.h: pmx_backward_trunk)
//   conv1_wgrad  dw[64][3][3][3] of conv1_1 from g (ldg >= 64 floats per pixel) and the prepared input x16 (PMX_IN_C floats per pixel);
//                ws: strips x 64 x 32 floats; (strips, rows) from conv1_wgrad_strips (forced <= 0: the rule)
//   maxpool      out [B][H/2][W/2][nch] = the 2 x 2 maximum of a [B][H][W][nch]
//   pool_bwd     g [B][H][W][nch] from u [B][H/2][W/2][nch] and a: u at the first maximum of each window where a > 0, +0.0f elsewhere
int conv1_wgrad_strips(int B, int H, int forced, int* rows);
int conv1_wgrad_launch(const float* g, int ldg, const float* x16, float* ws, float* dw, int B, int H, int W, int strips, int rows, hipStream_t stream);
int maxpool_nhwc_launch(const float* a, int lda, float* out, int ldo, int B, int H, int W, int nch, hipStream_t stream);
int pool_bwd_nhwc_launch(const float* u, int ldu, const float* a, int lda, float* g, int ldg, int B, int H, int W, int nch, hipStream_t stream);
// conv_bwd.hip: the elementwise steps of the head backward, NHWC (the sums' orders: include/pose_mi355x.h, pmx_backward_head)
//   mask       g = u where a > 0, +0.0f elsewhere, nch channels of every pixel (a null: g = u)
//   stage_sum  g [pixel][128] = loss_grad (+ d0 + d1: dx of the next stage's Mconv1_L1 / _L2 in concat-buffer order, both null for the last stage)
//   feat_sum   fg [pixel][128] = first ? a + b : (fg + a) + b
//   copy_cols  nch channels of every pixel from one leading dimension to another
int bwd_mask_nhwc_launch(const float* u, int ldu, const float* a, int lda, float* g, int ldg, long long npix, int nch, hipStream_t stream);
int bwd_stage_sum_launch(const float* lg, const float* d0, const float* d1, int ldd, float* g, long long npix, hipStream_t stream);
int bwd_feat_sum_launch(float* fg, const float* a, const float* b, int ld, int first, long long npix, hipStream_t stream);
int bwd_copy_cols_launch(const float* src, int lds, float* dst, int ldd, long long npix, int nch, hipStream_t stream);
// conv_bwd.hip: the range census of one g slice (pmx_backward_g_census): counts[0 .. 4] += the pixels' nch channels that are non-zero, flushed
// to zero by f16_rn_sat, f16 subnormals after it, above 65504 in magnitude, NaN.  counts: five device words, zeroed by the caller
int bwd_g_census_launch(const float* g, int ldg, long long npix, int nch, unsigned long long* counts, hipStream_t stream);
// pmx_api.hip, for pmx_backward.hip: one layer (pair) through the forward's dispatcher (run_conv: plan_conv + launch_plan), and the pack of
// c->bw.tl[layer] built from the layer's device weights (no-op when built)
// (precision: the call's, as FwdCall::precision -- 2 for a data gradient of the head chain under "grad_precision" 2; -1: the context's own)
int pmx_run_conv(pmx_ctx* c, const char* label, PackedLayer* L0, PackedLayer* L1, const ConvIO& io, int precision = -1);
int pmx_bw_transposed_pack(pmx_ctx* c, int layer, bool f16 = false);      // (f16: a 3x3 / 7x7 layer's f16 pack of it as well)
// c->smoothed (and c->pp.smoothed) at `floats` floats at least, grown to exactly that once the stream no longer uses the old maps
int pmx_ensure_smoothed(pmx_ctx* c, size_t floats);
// pmx_api.hip: the channel map kind of a layer's direct pack (pack_index.h).  pmx_train.hip: the master weights (w OIHW | b) of a layer with
// a segment while training is on (head; mode 2: trunk too), else null
int pmx_pack_kind(const pmx_ctx* c, int cin);
float* pmx_train_master(const pmx_ctx* c, int layer);
void pmx_train_free(pmx_ctx* c);
// pmx_packs.hip: the packers, the only way a pack gets built.  pmx_layer_geometry fills a layer's shape (cin_pad: pmx_pk_cin_pad of the
// layer's kind, pmx_pk_t_cin_pad for a transposed layer).  pmx_pack_job_* describe one pack to write (total set, blk0 = 0): the direct pack
// and bias of L from master weights; the transposed pack P of the layer (cout, cin, ks, kind) from its master weights; the f16, bf16x3 and
// Winograd packs and conv1_1's fused-kernel pack from L's direct pack into dst.  A job is enqueued alone (pmx_pack_launch_one, by value) or
// as one of a device table's (pmx_pack_launch_table: the jobs' blk0 ascending, `blocks` their sum).  pmx_unpack_launch: L's direct pack and
// bias -> (w OIHW | b).
// The kinds in launch order: what reads a direct pack comes after PMX_PACK_DIRECT.  PMX_PACK_JOBS_PER_LAYER: the jobs of a kind one layer
// gives a step's table at most (f16, Winograd: its own pack and its transposed layer's); 0: one job per context (conv1_1's).
enum { PMX_PACK_DIRECT = 0, PMX_PACK_F16, PMX_PACK_BF16X3, PMX_PACK_TRANSPOSED, PMX_PACK_WINO, PMX_PACK_CONV1, PMX_PACK_KINDS };
constexpr int PMX_PACK_JOBS_PER_LAYER[PMX_PACK_KINDS] = {1, 2, 1, 1, 2, 0};
void pmx_layer_geometry(PackedLayer& L, int cout, int cin, int ks, int cin_pad);
PackJob pmx_pack_job_direct(const float* master, const PackedLayer& L, int kind);
PackJob pmx_pack_job_f16(const PackedLayer& L, uint16_t* dst);
PackJob pmx_pack_job_bf16x3(const PackedLayer& L, uint16_t* dst);
PackJob pmx_pack_job_transposed(const float* master, int cout, int cin, int ks, int kind, const PackedLayer& P);
PackJob pmx_pack_job_wino(const PackedLayer& L, float* dst);
PackJob pmx_pack_job_conv1(const PackedLayer& L, float* dst);
int pmx_pack_launch_one(int kind, const PackJob& job, hipStream_t st);
int pmx_pack_launch_table(int kind, const PackJob* d_jobs, int njobs, unsigned blocks, hipStream_t st);
int pmx_unpack_launch(const PackedLayer& L, int kind, float* dst, hipStream_t st);
