// conv_f16.hip -- the opt-in f16 inference mode (option "precision" = 2; include/pose_mi355x.h): every 3x3 / 7x7
// convolution as a direct implicit GEMM on v_mfma_f32_32x32x16_f16.
//
// Contract, per output of a layer: y = sum over (chunk of 16 input channels, tap) of f16(x) . f16(w), accumulated in fp32 by ONE MFMA
// per (chunk, tap) in a fixed order -- chunk-major, taps row-major inside a chunk -- then the fp32 epilogue of every other kernel (2x2
// max-pool of the four sums, + bias, ReLU).  f16(v) = round-to-nearest-even, saturating at +-65504.  Nothing in that order depends on the
// launch: not on the batch, the image's position in it, the tile width in channels (BN) or the segment layout -- an image gives the same
// bits alone, anywhere in a uniform batch and inside a mixed-size batch.  No split-K.
//
// Geometry: a block = 8 x 16 output pixels (the PMX_SEG_RECT rectangles of the heterogeneous forward) x BN output channels, 256 threads.
// BN = 128: wave w owns channels [32 w, 32 w + 32) of all four 32-pixel MFMA tiles; BN = 64 (64-channel layers, small launches): 2 x 2
// waves of two tiles each.  MFMA row m of tile t <-> pixel of 2 x 2 window (8 t + m / 4): the pool happens on the four registers of a
// window, as in conv_direct.h.  Activations stay fp32 NHWC in HBM; the halo of one 16-channel chunk is converted to f16 while it is
// staged into LDS ([row][pixel][16 ch] f16, 32 bytes per pixel, rows padded by 16 bytes so that the two pixel rows a 16-lane group of
// ds_read_b128 touches fall on different bank halves: conflict-free), double-buffered, one barrier per chunk.  Weights (rounded once by
// the f16 packer of pmx_packs.hip, [tap][chunk][cout_pad][16] f16 = the fp32 pack's layout) come straight from L2, one tap ahead.
// LDS per MFMA (BN = 128): 1 KiB of A per wave and MFMA, 4 waves -> 4 KiB per 32 cycles = 128 B/clk/CU, half the 256 B/clk of ds_read_b128.
#include "conv_direct.h"
#include "f16_sat.h"

template <int KS>
struct F16Cfg {
    static constexpr int TH = 8, TW = 16, CK = 16, T = KS * KS, PADK = KS / 2;
    static constexpr int HALO_H = TH + KS - 1, HALO_W = TW + KS - 1;
    static constexpr int RP = HALO_W * 32 + 16;                         // bytes per halo row
    static constexpr int BUF = HALO_H * RP;                             // bytes per halo buffer
    static constexpr int UNITS = HALO_H * HALO_W * (CK / 4);            // float4 units of one chunk's halo
    static constexpr int NHF = (UNITS + 255) / 256;
};

// (the fp32 -> f16 conversion of the staged halo: f16_sat.h::f16_sat4)
template <int KS, typename OP, int BN>
__global__ __launch_bounds__(256, 2) void conv_f16_kernel(const ConvArgs a)
{
    using C = F16Cfg<KS>;
    constexpr int WN = BN / 32, WM = 4 / WN, MT = 4 / WM;              // waves over channels / pixels, 32-pixel tiles per wave
    constexpr int RP = C::RP, T = C::T;
    extern __shared__ float4 smem4[];
    char* const s_in = reinterpret_cast<char*>(smem4);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 31, kh = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const bool g1 = blockIdx.z != 0;
    const float* gin = g1 ? a.g[1].in : a.g[0].in;
    const OP* gw = reinterpret_cast<const OP*>(g1 ? a.g[1].w : a.g[0].w);     // f16 pack of the layer (passed in place of the fp32 pack)
    const float* gbias = g1 ? a.g[1].bias : a.g[0].bias;
    float* gout = g1 ? a.g[1].out : a.g[0].out;
    const int cout = g1 ? a.g[1].cout : a.g[0].cout;

    // tile -> (segment,) image, rectangle.  Heterogeneous launches: segment s owns tiles [segs[s].tile0, segs[s + 1].tile0)
    int tile = blockIdx.x;
    int H = a.H, W = a.W, tiles_x = a.tiles_x, tiles_img = a.tiles_x * a.tiles_y;
    size_t pix_in = 0, pix_out = 0;
    if (a.nseg > 0) {
        int sg = 0;
        for (int k = 1; k < a.nseg; ++k) sg = tile >= a.segs[k].tile0 ? k : sg;
        const ConvSeg S = a.segs[sg];
        H = S.H; W = S.W; tiles_x = S.tiles_x; tiles_img = S.tiles_img;
        pix_in = (size_t)(unsigned)S.pix0; pix_out = (size_t)(unsigned)S.pixo;
        tile -= S.tile0;
    }
    const int bimg = tile / tiles_img, trem = tile - bimg * tiles_img;
    const int y0 = (trem / tiles_x) * C::TH, x0 = (trem % tiles_x) * C::TW;
    const int Ho = a.pool ? H >> 1 : H, Wo = a.pool ? W >> 1 : W;
    const float* in_b = gin + (pix_in + (size_t)bimg * H * W) * a.lda;
    float* out_b = gout + (pix_out + (size_t)bimg * Ho * Wo) * a.ldc;
    const int n = blockIdx.y * BN + wn * 32 + li;
    const float bias = gbias[n];                          // (bias is padded to cout_pad)

    // LDS byte offset of this lane's A row (pixel) in each of its tiles, tap (0, 0)
    int a_off[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = (wm * MT + t) * 32 + li, q = m >> 2, r = m & 3;
        const int py = 2 * (q / (C::TW / 2)) + (r >> 1), px = 2 * (q % (C::TW / 2)) + (r & 1);
        a_off[t] = py * RP + px * 32 + kh * 16;
    }
    // halo staging: unit f = (halo pixel, 4 channels)
    int h_goff[C::NHF], h_lds[C::NHF];
    unsigned h_ok = 0;
#pragma unroll
    for (int r = 0; r < C::NHF; ++r) {
        const int f = tid + r * 256;
        const bool slot = f < C::UNITS;
        const int hp = slot ? f >> 2 : 0, c4 = f & 3;
        const int hy = hp / C::HALO_W, hx = hp - hy * C::HALO_W;
        const int gy = y0 + hy - C::PADK, gx = x0 + hx - C::PADK;
        const bool inb = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
        h_goff[r] = inb ? (gy * W + gx) * a.lda + c4 * 4 : 0;
        h_lds[r] = slot ? hy * RP + hx * 32 + c4 * 8 : -1;
        h_ok |= (slot && inb) ? (1u << r) : 0u;
    }
    auto halo_load = [&](float4 (&hv)[C::NHF], int ch) {
#pragma unroll
        for (int r = 0; r < C::NHF; ++r)
            hv[r] = ((h_ok >> r) & 1) ? *reinterpret_cast<const float4*>(in_b + h_goff[r] + ch * C::CK) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto halo_store = [&](char* buf, const float4 (&hv)[C::NHF]) {
#pragma unroll
        for (int r = 0; r < C::NHF; ++r) {
            if (h_lds[r] < 0) continue;
            *reinterpret_cast<f16x4*>(buf + h_lds[r]) = f16_sat4(hv[r]);
        }
    };

    f32x16 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    // weights of (tap, chunk): 16 bytes per lane at [tap][chunk][n][kh * 8 .. kh * 8 + 7]
    const size_t w_lane = (size_t)n * C::CK + kh * 8;
    const size_t w_tap = (size_t)a.nch * a.cout_pad * C::CK, w_chunk = (size_t)a.cout_pad * C::CK;
    auto load_b = [&](int ch, int tap) { return *reinterpret_cast<const f16x8*>(gw + w_lane + (size_t)tap * w_tap + (size_t)ch * w_chunk); };

    {
        float4 hv[C::NHF];
        halo_load(hv, 0);
        halo_store(s_in, hv);
    }
    __syncthreads();

    f16x8 bc = load_b(0, 0);
    for (int ch = 0; ch < a.nch; ++ch) {
        const char* cur = s_in + (ch & 1) * C::BUF;
        char* nxt = s_in + ((ch + 1) & 1) * C::BUF;
        const bool more = ch + 1 < a.nch;
        float4 hreg[C::NHF];
        if (more) halo_load(hreg, ch + 1);               // next chunk's halo: global -> registers under this chunk's MFMAs
#pragma unroll 1
        for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
            for (int kx = 0; kx < KS; ++kx) {
                const int tap = ky * KS + kx;
                // next (tap, chunk) in the K order: the following tap, or tap 0 of the next chunk (the very last: itself again)
                const f16x8 bn = tap + 1 < T ? load_b(ch, tap + 1) : load_b(more ? ch + 1 : ch, 0);
                f16x8 av[MT];
#pragma unroll
                for (int t = 0; t < MT; ++t) av[t] = *reinterpret_cast<const f16x8*>(cur + a_off[t] + ky * RP + kx * 32);
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[t], bc, acc[t], 0, 0, 0);
                bc = bn;
            }
        }
        if (more) {
            halo_store(nxt, hreg);                       // (the other buffer: its last readers passed the previous barrier)
            __syncthreads();
        }
    }

    // epilogue: (2x2 max-pool,) + bias, ReLU, masked NHWC store.  C/D layout: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 kh
    const bool nok = n < cout;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int tm = wm * MT + t;
        if (!a.pool) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int q = tm * 8 + 2 * (reg >> 2) + kh, r = reg & 3;
                const int gy = y0 + 2 * (q / (C::TW / 2)) + (r >> 1), gx = x0 + 2 * (q % (C::TW / 2)) + (r & 1);
                float v = acc[t][reg] + bias;
                if (a.relu) v = pmx_relu_nan(v);
                if (nok && gy < H && gx < W) out_b[(size_t)(gy * W + gx) * a.ldc + n] = v;
            }
        } else {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                float v = pmx_max4_nan(acc[t][4 * g4 + 0], acc[t][4 * g4 + 1], acc[t][4 * g4 + 2], acc[t][4 * g4 + 3]);
                v += bias;
                if (a.relu) v = pmx_relu_nan(v);
                const int q = tm * 8 + 2 * g4 + kh;
                const int oy = (y0 >> 1) + q / (C::TW / 2), ox = (x0 >> 1) + q % (C::TW / 2);
                if (nok && oy < Ho && ox < Wo) out_b[(size_t)(oy * Wo + ox) * a.ldc + n] = v;
            }
        }
    }
}

template <int KS, int BN>
static int launch_f16(const ConvArgs& a0, int groups, hipStream_t stream)
{
    using C = F16Cfg<KS>;
    ConvArgs a = a0;
    a.tiles_x = (a.W + C::TW - 1) / C::TW;
    a.tiles_y = (a.H + C::TH - 1) / C::TH;
    auto kern = conv_f16_kernel<KS, _Float16, BN>;
    const unsigned gx = a.nseg ? (unsigned)a.seg_tiles : (unsigned)(a.tiles_x * a.tiles_y * a.B);
    hipLaunchKernelGGL(kern, dim3(gx, (unsigned)(a.cout_pad / BN), (unsigned)groups), dim3(256), 2 * C::BUF, stream, a);
    PMX_HIP(hipGetLastError());
    return PMX_OK;
}

// 8 x 16 pixel tiles of a launch (the segment table's count in a heterogeneous forward)
long long conv_f16_tiles(const ConvArgs& a)
{
    return a.nseg ? a.seg_tiles : (long long)a.B * ((a.W + 15) / 16) * ((a.H + 7) / 8);
}

// blocks of 128 channels where the launch fills the chip with them, else 64 (the per-output K order is the same either way).  f16_bn: the
// context's option "f16_bn" -- 0 = that rule, 64 | 128 = that width instead of the rule's answer (128 only where the layer has blocks of 128)
int conv_f16_bn(const ConvArgs& a, int groups, int f16_bn, int ncu)
{
    if (a.cout_pad % 128) return 64;
    if (f16_bn) return f16_bn;
    return conv_f16_tiles(a) * (a.cout_pad / 128) * groups >= ncu ? 128 : 64;
}

int conv_f16_launch(int ks, const ConvArgs& a, int groups, int f16_bn, int ncu, hipStream_t stream)
{
    PMX_CHECK(ks == 3 || ks == 7, PMX_ERR_INVALID, "conv f16: kernel size %d (3 or 7)", ks);
    PMX_CHECK(groups == 1 || groups == 2, PMX_ERR_INVALID, "conv f16: %d groups", groups);
    PMX_CHECK(a.cout_pad % 64 == 0, PMX_ERR_INVALID, "conv f16: cout_pad %d not a multiple of 64", a.cout_pad);
    PMX_CHECK(a.lda % 4 == 0 && a.nch >= 1 && a.nch * 16 <= a.lda, PMX_ERR_INVALID, "conv f16: %d chunks over a channel stride of %d", a.nch, a.lda);
    PMX_CHECK(a.nseg > 0 ? (a.segs != nullptr && a.seg_tiles > 0) : a.B >= 1, PMX_ERR_INVALID, "conv f16: empty launch");
    PMX_CHECK(!a.pool || (a.H % 2 == 0 && a.W % 2 == 0), PMX_ERR_INVALID, "conv f16: pooled layer needs even H, W");
    PMX_CHECK((long long)a.H * a.W * a.lda < (1ll << 31) && (long long)a.H * a.W * a.ldc < (1ll << 31), PMX_ERR_INVALID,
              "conv f16: image too large for 32-bit offsets");
    PMX_CHECK(f16_bn == 0 || f16_bn == 64 || f16_bn == 128, PMX_ERR_INVALID, "conv f16: block width %d (0, 64 or 128)", f16_bn);
    const int bn = conv_f16_bn(a, groups, f16_bn, ncu);
    if (ks == 7) return bn == 128 ? launch_f16<7, 128>(a, groups, stream) : launch_f16<7, 64>(a, groups, stream);
    return bn == 128 ? launch_f16<3, 128>(a, groups, stream) : launch_f16<3, 64>(a, groups, stream);
}
