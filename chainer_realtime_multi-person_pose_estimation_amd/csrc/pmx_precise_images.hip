// pmx_precise_images.hip -- detect_precise (reference pose_detector.py:433-482) for a LIST of images of any sizes in one call
// (include/pose_mi355x.h: pmx_detect_precise_images, pmx_get_precise_image_maps, pmx_precise_images_table_bytes).
// Every (image, scale) pair of the call is one segment of ONE network forward on the context's stream (pmx_multi.hip's segment tables;
// pairs of equal network size are adjacent and merge into one segment, the largest first).  Around it three segment-aware kernels, each
// one launch over all pairs / images of the call with a small device table for the block -> pair / image lookup:
//   pi_input_kernel    u8 cubic resize to the scaled size + pad to a multiple of 8 with (104, 117, 123) (or the copy of a scale whose size
//                      is the original's) = resize_cubic_u8_kernel + fill_pad_bgr_kernel (+ the copy) of pmx_precise.hip, per pixel
//   pi_upsample_kernel x8 cubic up-sampling of the 38 PAF + 19 heat channels of the NHWC cat buffer into planar temporaries
//                      = resize_cubic_f32_rows_kernel (prep.hip) on each pair
//   pi_average_kernel  crop + cubic resize to the original size of every scale IN SLOT ORDER, summed from 0.f and divided by the number of
//                      scales, straight into the full-resolution maps = resize_cubic_f32_rows_kernel per scale + sum_parts_f32_kernel,
//                      without the per-scale full-resolution parts
// Same float32 operations in the same order as the kernels they replace (this file is compiled with -ffp-contract=off like prep.hip), so
// the maps are bit-identical to the begin / add_scale / finish sequence run image by image with the same network kernels.  The post-process
// runs per run of equal original sizes on its view of the post-process buffers, as pmx_postprocess_images does.  All tables of a call
// (cubic tables, post-process grids, descriptors) are built on the host and go over in ONE copy into a per-call buffer: no table is cached
// by size, so a data set with a new size every frame neither allocates nor synchronises per size.
#include "pmx_ctx.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <utility>

namespace {

constexpr int PI_CH = PMX_N_PAF + PMX_N_HEAT;     // 57 planes per map set: 38 PAF, then 19 heat
constexpr int PI_RB = 16, PI_NR = 32;             // destination rows per block, LDS rows (launch_resize_cubic_f32_planar's rows form)
constexpr int PI_MAX_SCALES = 8;

// one (image, scale) pair = one network input of the call
struct PiPair {
    long long src;        // first byte of the image's original pixels in pi_src
    long long dst;        // first byte of the padded network input in the uint8 run (segment order)
    long long pix0;       // first padded pixel of the pair in pi_input_kernel's flat index space
    long long cat_pix;    // first level-3 pixel of the pair in the cat buffer
    long long tmp;        // first float of the pair's planar temporaries [57][ph][pw]
    int sh, sw;           // original size
    int dh, dw;           // scaled size
    int ph, pw;           // padded network size
    int same;             // scaled size == original size: a copy (cv2.resize identity)
    int tab_u8;           // int offset of the u8 tables [x: 8 dw | y: 8 dh] (fixed point)
    int tab_up;           // int offset of the x8 up-sampling tables [x: 8 pw | y: 8 ph]
    int blk;              // first block of the pair in pi_upsample_kernel's grid
};
// one image of the call
struct PiImage {
    long long out;        // first float of the image's full-resolution maps [57][oh][ow]
    int oh, ow, ns;       // original size, number of scales
    int blk;              // first block of the image in pi_average_kernel's grid
    int pair[PI_MAX_SCALES];     // pair of scale slot k
    int tab_dn[PI_MAX_SCALES];   // int offset of the tables (scaled -> original) of slot k [x: 8 ow | y: 8 oh]
};

// last entry e of a non-decreasing key array with key(e) <= v (block-uniform: the loads are scalar)
template <typename T, typename K>
__device__ inline int find_entry(const T* __restrict__ a, int n, K key, long long v)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((long long)key(a[mid]) <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void pi_input_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const PiPair* __restrict__ pairs,
                                                       int npairs, const int* __restrict__ tab, long long npix)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const PiPair& P = pairs[find_entry(pairs, npairs, [](const PiPair& q) { return q.pix0; }, i)];
    const int p = (int)(i - P.pix0);
    const int y = p / P.pw, x = p - y * P.pw;
    uint8_t* const o = dst + P.dst + (long long)p * 3;
    if (y >= P.dh || x >= P.dw) {                 // fill_pad_bgr_kernel
        o[0] = (uint8_t)104; o[1] = (uint8_t)117; o[2] = (uint8_t)123;
        return;
    }
    const uint8_t* const s = src + P.src;
    if (P.same) {
        const uint8_t* q = s + ((long long)y * P.sw + x) * 3;
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
        return;
    }
    // resize_cubic_u8_kernel
    const int dw = P.dw, dh = P.dh, sw = P.sw;
    const int* xi = tab + P.tab_u8;
    const int* xa = xi + 4 * dw;
    const int* yi = xa + 4 * dw;
    const int* ya = yi + 4 * dh;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        long long acc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint8_t* r = s + ((long long)yi[k * dh + y] * sw) * 3 + c;
            const long long row = (long long)r[xi[x] * 3] * xa[x] + (long long)r[xi[dw + x] * 3] * xa[dw + x] +
                                  (long long)r[xi[2 * dw + x] * 3] * xa[2 * dw + x] + (long long)r[xi[3 * dw + x] * 3] * xa[3 * dw + x];
            acc += row * ya[k * dh + y];
        }
        long long v = (acc + (1ll << 21)) >> 22;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
        o[c] = (uint8_t)v;
    }
}

// The separable cubic resize of resize_cubic_f32_rows_kernel for the destination rows y0 .. y1 (at most PI_RB) at column x of one plane:
// the horizontal 4-tap sums of the source rows the block touches go to this thread's own LDS column (no other thread reads it), then every
// row takes its four sums from there; emit(r, v) receives row y0 + r.  Same float32 operations in the same order.
template <typename F>
__device__ inline void cubic_rows(float* sH, int tid, const float* __restrict__ s, long long sy, long long sx, int dh, int dw, int x, int y0, int y1,
                                  const int* __restrict__ xi, const float* __restrict__ xc, const int* __restrict__ yi, const float* __restrict__ yc, F emit)
{
    const int r_lo = yi[y0], r_hi = yi[3 * dh + y1];          // (tap indices are clamped and non-decreasing in k and y)
    const int nrows = r_hi - r_lo + 1;
    const long long x0 = (long long)xi[x] * sx, x1 = (long long)xi[dw + x] * sx, x2 = (long long)xi[2 * dw + x] * sx, x3 = (long long)xi[3 * dw + x] * sx;
    const float c0 = xc[x], c1 = xc[dw + x], c2 = xc[2 * dw + x], c3 = xc[3 * dw + x];
    auto hsum = [&](int sr) -> float {
        const float* r = s + (long long)sr * sy;
        float a = r[x0] * c0;
        a = a + r[x1] * c1;
        a = a + r[x2] * c2;
        a = a + r[x3] * c3;
        return a;
    };
    const bool lds = nrows <= PI_NR;
    if (lds) {
        for (int r = 0; r < nrows; ++r) sH[r * 256 + tid] = hsum(r_lo + r);
    }
#pragma unroll
    for (int r = 0; r < PI_RB; ++r) {
        const int y = y0 + r;
        if (y > y1) break;
        float h0, h1, h2, h3;
        if (lds) {
            h0 = sH[(yi[y] - r_lo) * 256 + tid]; h1 = sH[(yi[dh + y] - r_lo) * 256 + tid];
            h2 = sH[(yi[2 * dh + y] - r_lo) * 256 + tid]; h3 = sH[(yi[3 * dh + y] - r_lo) * 256 + tid];
        } else {
            h0 = hsum(yi[y]); h1 = hsum(yi[dh + y]); h2 = hsum(yi[2 * dh + y]); h3 = hsum(yi[3 * dh + y]);
        }
        float v = h0 * yc[y];
        v = v + h1 * yc[dh + y];
        v = v + h2 * yc[2 * dh + y];
        v = v + h3 * yc[3 * dh + y];
        emit(r, v);
    }
}

__device__ inline long long cat_channel(int plane) { return plane < PMX_N_PAF ? PMX_CAT_PAF + plane : PMX_CAT_HEAT + (plane - PMX_N_PAF); }

// grid: the blocks of all pairs; a pair's blocks are (x / 256 fastest, then rows / PI_RB, then plane) of its ph x pw up-sampled planes
__global__ __launch_bounds__(256) void pi_upsample_kernel(const float* __restrict__ cat, float* __restrict__ tmp, const PiPair* __restrict__ pairs,
                                                          int npairs, const int* __restrict__ tab)
{
    __shared__ float sH[PI_NR * 256];
    const int tid = (int)threadIdx.x;
    const PiPair& P = pairs[find_entry(pairs, npairs, [](const PiPair& q) { return q.blk; }, (long long)blockIdx.x)];
    const int ph = P.ph, pw = P.pw, fw = pw / 8;
    const int bx = (pw + 255) / 256, by = (ph + PI_RB - 1) / PI_RB;
    const int local = (int)blockIdx.x - P.blk, plane = local / (bx * by), rem = local - plane * bx * by;
    const int ty = rem / bx, tx = rem - ty * bx;
    const int x = tx * 256 + tid;
    if (x >= pw) return;
    const int y0 = ty * PI_RB, y1 = min(y0 + PI_RB, ph) - 1;
    const float* s = cat + P.cat_pix * PMX_CAT_C + cat_channel(plane);
    float* d = tmp + P.tmp + (long long)plane * ph * pw;
    const int* xi = tab + P.tab_up;
    const float* xc = reinterpret_cast<const float*>(xi + 4 * pw);
    const int* yi = xi + 8 * pw;
    const float* yc = reinterpret_cast<const float*>(yi + 4 * ph);
    cubic_rows(sH, tid, s, (long long)fw * PMX_CAT_C, PMX_CAT_C, ph, pw, x, y0, y1, xi, xc, yi, yc,
               [&](int r, float v) { d[(long long)(y0 + r) * pw + x] = v; });
}

// grid: the blocks of all images; an image's blocks are (x / 256 fastest, then rows / PI_RB, then plane) of its oh x ow maps
__global__ __launch_bounds__(256) void pi_average_kernel(const float* __restrict__ tmp, float* __restrict__ maps, const PiPair* __restrict__ pairs,
                                                         const PiImage* __restrict__ imgs, int nimg, const int* __restrict__ tab)
{
    __shared__ float sH[PI_NR * 256];
    const int tid = (int)threadIdx.x;
    const PiImage& I = imgs[find_entry(imgs, nimg, [](const PiImage& q) { return q.blk; }, (long long)blockIdx.x)];
    const int oh = I.oh, ow = I.ow;
    const int bx = (ow + 255) / 256, by = (oh + PI_RB - 1) / PI_RB;
    const int local = (int)blockIdx.x - I.blk, plane = local / (bx * by), rem = local - plane * bx * by;
    const int ty = rem / bx, tx = rem - ty * bx;
    const int x = tx * 256 + tid;
    if (x >= ow) return;
    const int y0 = ty * PI_RB, y1 = min(y0 + PI_RB, oh) - 1;
    float acc[PI_RB];
#pragma unroll
    for (int r = 0; r < PI_RB; ++r) acc[r] = 0.f;
    const int ns = I.ns;
    for (int k = 0; k < ns; ++k) {                // slot order: the reference's `sum = sum + resized` (:463,467)
        const PiPair& P = pairs[I.pair[k]];
        const float* s = tmp + P.tmp + (long long)plane * P.ph * P.pw;      // (the crop: the tables index rows < dh, columns < dw only)
        const int* xi = tab + I.tab_dn[k];
        const float* xc = reinterpret_cast<const float*>(xi + 4 * ow);
        const int* yi = xi + 8 * ow;
        const float* yc = reinterpret_cast<const float*>(yi + 4 * oh);
        cubic_rows(sH, tid, s, P.pw, 1, oh, ow, x, y0, y1, xi, xc, yi, yc, [&](int r, float v) { acc[r] = acc[r] + v; });
    }
    const float divisor = (float)ns;
    float* d = maps + I.out + (long long)plane * oh * ow;
#pragma unroll
    for (int r = 0; r < PI_RB; ++r) {
        if (y0 + r > y1) break;
        d[(long long)(y0 + r) * ow + x] = acc[r] / divisor;        // (:469-470)
    }
}

struct HostPair { int img, slot, ph, pw; };

}  // namespace

extern "C" int pmx_detect_precise_images(pmx_ctx* c, const pmx_precise_image* imgs, int n)
{
    PMX_CHECK(c && imgs, PMX_ERR_INVALID, "pmx_detect_precise_images: null arg");
    PMX_CHECK(c->kind == NET_POSE, PMX_ERR_STATE, "pmx_detect_precise_images: posenet contexts only");
    PMX_LOSS_NO_MIXED(c, "pmx_detect_precise_images");
    PMX_CHECK(n >= 1 && n <= c->max_batch, PMX_ERR_CAPACITY, "pmx_detect_precise_images: %d images outside 1..%d (the context's batch capacity)", n,
              c->max_batch);
    PMX_CHECK(c->opt_precision == 0 || c->opt_precision == 2, PMX_ERR_INVALID,
              "pmx_detect_precise_images: option \"precision\" = %d has no segment form (the bf16x3 kernels); use 0 (fp32) or 2 (f16)", c->opt_precision);
    PMX_CHECK(!c->opt_keep_smoothed, PMX_ERR_STATE, "pmx_detect_precise_images: option keep_smoothed is not available for image lists");
    int rc = pmx_check_weights(c);
    if (rc) return rc;
    // ---- the pairs, validated and sized: everything below is checked before anything is enqueued
    std::vector<HostPair> hp;
    long long src_bytes = 0, maps_floats = 0;
    for (int i = 0; i < n; ++i) {
        const pmx_precise_image& m = imgs[i];
        PMX_CHECK(m.bgr && m.orig_h >= 1 && m.orig_w >= 1, PMX_ERR_INVALID, "pmx_detect_precise_images: image %d: bad descriptor", i);
        PMX_CHECK(m.n_scales >= 1 && m.n_scales <= PI_MAX_SCALES, PMX_ERR_INVALID, "pmx_detect_precise_images: image %d: %d scales outside 1..%d", i,
                  m.n_scales, PI_MAX_SCALES);
        PMX_CHECK((long long)m.orig_h * m.orig_w < (1ll << 31) / 256, PMX_ERR_CAPACITY,
                  "pmx_detect_precise_images: image %d: full-resolution maps of %d x %d exceed the 32-bit offsets of the post-process", i, m.orig_h, m.orig_w);
        for (int k = 0; k < m.n_scales; ++k) {
            const int sh = m.scaled_hw[2 * k], sw = m.scaled_hw[2 * k + 1];
            PMX_CHECK(sh >= 1 && sw >= 1 && sh <= (1 << 16) && sw <= (1 << 16), PMX_ERR_INVALID, "pmx_detect_precise_images: image %d scale %d: bad size %d x %d",
                      i, k, sh, sw);
            const int ph = round_up(sh, 8), pw = round_up(sw, 8);
            PMX_CHECK((long long)ph * pw * 64 * 4 < (1ll << 31), PMX_ERR_CAPACITY,
                      "pmx_detect_precise_images: image %d scale %d: network input %d x %d too large for the 32-bit buffer extents of the convolutions", i, k, ph, pw);
            hp.push_back(HostPair{i, k, ph, pw});
        }
        src_bytes += (long long)m.orig_h * m.orig_w * 3;
        maps_floats += (long long)PI_CH * m.orig_h * m.orig_w;
    }
    // equal network sizes adjacent (one segment), the largest first (the last, part-filled round of the CUs then holds small tiles)
    std::stable_sort(hp.begin(), hp.end(), [](const HostPair& a, const HostPair& b) {
        const long long pa = (long long)a.ph * a.pw, pb = (long long)b.ph * b.pw;
        if (pa != pb) return pa > pb;
        if (a.ph != b.ph) return a.ph > b.ph;
        return a.pw > b.pw;
    });
    const int np = (int)hp.size();
    long long px0 = 0, px3 = 0, tmp_floats = 0, up_blocks = 0, dn_blocks = 0;
    for (const HostPair& q : hp) {
        px0 += (long long)q.ph * q.pw;
        px3 += (long long)(q.ph / 8) * (q.pw / 8);
        tmp_floats += (long long)PI_CH * q.ph * q.pw;
        up_blocks += (long long)PI_CH * ((q.pw + 255) / 256) * ((q.ph + PI_RB - 1) / PI_RB);
    }
    for (int i = 0; i < n; ++i) dn_blocks += (long long)PI_CH * ((imgs[i].orig_w + 255) / 256) * ((imgs[i].orig_h + PI_RB - 1) / PI_RB);
    const long long cap0 = (long long)c->max_batch * c->max_h * c->max_w, cap3 = (long long)c->max_batch * ((long long)c->max_h * c->max_w / 64);
    PMX_CHECK(px0 <= cap0, PMX_ERR_CAPACITY, "pmx_detect_precise_images: %lld network-input pixels of %d (image, scale) pairs exceed the context capacity %d x %d x %d",
              px0, np, c->max_batch, c->max_h, c->max_w);
    PMX_CHECK(px3 <= cap3, PMX_ERR_CAPACITY, "pmx_detect_precise_images: %lld level-3 pixels (cat / br* buffers) exceed the context's %lld", px3, cap3);
    PMX_CHECK(px0 < (1ll << 31), PMX_ERR_CAPACITY, "pmx_detect_precise_images: %lld network-input pixels exceed the 31-bit pixel offsets of the segment tables", px0);
    PMX_CHECK(tmp_floats < (1ll << 40) && up_blocks < (1ll << 31), PMX_ERR_CAPACITY,
              "pmx_detect_precise_images: planar temporaries of %lld floats / %lld blocks too large", tmp_floats, up_blocks);
    PMX_CHECK(maps_floats < (1ll << 40) && dn_blocks < (1ll << 31), PMX_ERR_CAPACITY,
              "pmx_detect_precise_images: full-resolution maps of %lld floats / %lld blocks too large", maps_floats, dn_blocks);

    // ---- host staging: [pairs | images | int tables | post-process taps, grids (pp_tables.h)]
    std::vector<PiPair> pairs(np);
    std::vector<PiImage> pim(n);
    std::vector<SegGeo> segs;
    std::vector<int> itab;
    std::vector<long long> src_off(n);
    {
        long long so = 0;
        for (int i = 0; i < n; ++i) { src_off[i] = so; so += (long long)imgs[i].orig_h * imgs[i].orig_w * 3; }
    }
    auto add_table = [&](int src, int dst, bool fixed) {
        const size_t o = itab.size();
        itab.resize(o + (size_t)8 * dst);
        pmx_cubic_table(src, dst, fixed, itab.data() + o);
        return (long long)o;
    };
    long long off_pix = 0, off3 = 0, off_tmp = 0, blk = 0, max_tab = 0;
    for (int j = 0; j < np; ++j) {
        const HostPair& q = hp[j];
        const pmx_precise_image& m = imgs[q.img];
        PiPair& P = pairs[j];
        P.sh = m.orig_h; P.sw = m.orig_w;
        P.dh = m.scaled_hw[2 * q.slot]; P.dw = m.scaled_hw[2 * q.slot + 1];
        P.ph = q.ph; P.pw = q.pw;
        P.same = P.dh == P.sh && P.dw == P.sw;
        P.src = src_off[q.img];
        P.pix0 = off_pix; P.dst = off_pix * 3; P.cat_pix = off3; P.tmp = off_tmp; P.blk = (int)blk;
        P.tab_u8 = 0;
        if (!P.same) {
            const long long t = add_table(P.sw, P.dw, true);
            add_table(P.sh, P.dh, true);
            P.tab_u8 = (int)t; max_tab = std::max(max_tab, t);
        }
        const long long t = add_table(q.pw / 8, q.pw, false);
        add_table(q.ph / 8, q.ph, false);
        P.tab_up = (int)t; max_tab = std::max(max_tab, t);
        off_pix += (long long)q.ph * q.pw; off3 += (long long)(q.ph / 8) * (q.pw / 8); off_tmp += (long long)PI_CH * q.ph * q.pw;
        blk += (long long)PI_CH * ((q.pw + 255) / 256) * ((q.ph + PI_RB - 1) / PI_RB);
        if (!segs.empty() && segs.back().H == q.ph && segs.back().W == q.pw) segs.back().n += 1;
        else segs.push_back(SegGeo{1, q.ph, q.pw, 0, 0});
        pim[q.img].pair[q.slot] = j;
    }
    {
        long long out = 0, b = 0;
        for (int i = 0; i < n; ++i) {
            const pmx_precise_image& m = imgs[i];
            PiImage& I = pim[i];
            I.out = out; I.oh = m.orig_h; I.ow = m.orig_w; I.ns = m.n_scales; I.blk = (int)b;
            for (int k = 0; k < PI_MAX_SCALES; ++k) {
                if (k >= m.n_scales) { I.pair[k] = 0; I.tab_dn[k] = 0; continue; }
                const long long t = add_table(m.scaled_hw[2 * k + 1], m.orig_w, false);
                add_table(m.scaled_hw[2 * k], m.orig_h, false);
                I.tab_dn[k] = (int)t; max_tab = std::max(max_tab, t);
            }
            out += (long long)PI_CH * m.orig_h * m.orig_w;
            b += (long long)PI_CH * ((m.orig_w + 255) / 256) * ((m.orig_h + PI_RB - 1) / PI_RB);
        }
    }
    PMX_CHECK(itab.size() < (1ull << 31), PMX_ERR_CAPACITY, "pmx_detect_precise_images: %zu table ints exceed the 32-bit table offsets", itab.size());
    // post-process tables (pp_tables.h): one taps block, then one grid per distinct original size (the identity up-sampling of
    // pmx_postprocess at full resolution)
    std::map<std::pair<int, int>, PPTables> tab_of;      // (oh, ow) -> its table set; the grids lie in the order of this map
    size_t pp_bytes = pp_taps_bytes();
    for (int i = 0; i < n; ++i)
        if (tab_of.emplace(std::make_pair(imgs[i].orig_h, imgs[i].orig_w), PPTables{}).second) pp_bytes += pp_grid_bytes(imgs[i].orig_h, imgs[i].orig_w);
    const size_t o_pairs = 0, o_imgs = o_pairs + ((size_t)np * sizeof(PiPair) + 15) / 16 * 16;
    const size_t o_tab = o_imgs + ((size_t)n * sizeof(PiImage) + 15) / 16 * 16;
    const size_t o_pp = o_tab + (itab.size() * sizeof(int) + 15) / 16 * 16;
    const size_t total = o_pp + pp_bytes;

    // ---- device buffers (grown on demand; the context's own buffers were checked above)
    PMX_DEV(c);
    // a buffer too small grows to a quarter more than asked (launches of the previous call may still read the old one: ensure synchronises)
    auto grow = [c](auto& b, size_t need) { return need <= b.capacity() ? PMX_OK : b.ensure(need + need / 4, c->stream); };
    if ((rc = grow(c->pi_dev, total)) || (rc = grow(c->pi_src, (size_t)src_bytes)) || (rc = grow(c->pi_tmp, (size_t)tmp_floats)) ||
        (rc = grow(c->pi_maps, (size_t)maps_floats)))
        return rc;
    // (the tables hold device addresses: filled once pi_dev is where this call's copy will lie)
    std::vector<double> stage((total + 7) / 8);
    char* const hs = reinterpret_cast<char*>(stage.data());
    memcpy(hs + o_pairs, pairs.data(), (size_t)np * sizeof(PiPair));
    memcpy(hs + o_imgs, pim.data(), (size_t)n * sizeof(PiImage));
    memcpy(hs + o_tab, itab.data(), itab.size() * sizeof(int));
    PPTables taps{};
    pmx_pp_gauss(c, hs + o_pp, c->pi_dev + o_pp, taps);
    size_t o_grid = o_pp + pp_taps_bytes();
    for (auto& g : tab_of) {
        const int oh = g.first.first, ow = g.first.second;
        g.second = taps;
        pp_grid_build(oh, ow, oh, ow, 0, hs + o_grid, c->pi_dev + o_grid, g.second);
        o_grid += pp_grid_bytes(oh, ow);
    }
    const PiPair* d_pairs = reinterpret_cast<const PiPair*>(c->pi_dev + o_pairs);
    const PiImage* d_imgs = reinterpret_cast<const PiImage*>(c->pi_dev + o_imgs);
    const int* d_tab = reinterpret_cast<const int*>(c->pi_dev + o_tab);
    // (stream-ordered after every launch of an earlier call; the host memory is read before build_seg_tables' synchronisation returns)
    c->pp_valid = false;
    c->pp_calls.clear();
    auto enqueue = [&]() -> int {
        PMX_HIP(hipMemcpyAsync(c->pi_dev, hs, total, hipMemcpyHostToDevice, c->stream));
        for (int i = 0; i < n; ++i)
            PMX_HIP(hipMemcpyAsync(c->pi_src + src_off[i], imgs[i].bgr, (size_t)imgs[i].orig_h * imgs[i].orig_w * 3, hipMemcpyHostToDevice, c->stream));
        int r;
        if ((r = pmx_prof_begin(c, "precise_input|pi_input_kernel", (double)px0 * 3 * 2))) return r;
        hipLaunchKernelGGL(pi_input_kernel, dim3((unsigned)((px0 + 255) / 256)), dim3(256), 0, c->stream, c->pi_src.get(), c->u8_tmp.get(), d_pairs, np, d_tab, px0);
        PMX_HIP(hipGetLastError());
        return pmx_prof_end(c);
    };
    if ((rc = enqueue())) { (void)hipStreamSynchronize(c->stream); return rc; }
    // ---- the network over all pairs (one launch per layer; build_seg_tables synchronises once)
    rc = forward_segments(c, c->u8_tmp, segs, np);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    c->maps_valid = false;                            // the cat buffer holds single scales: the averaged maps are pmx_get_precise_image_maps'
    c->cur_segs.clear();
    if ((rc = pmx_prof_begin(c, "precise_upsample|pi_upsample_kernel", (double)px3 * PI_CH * 4 + (double)tmp_floats * 4))) return rc;
    hipLaunchKernelGGL(pi_upsample_kernel, dim3((unsigned)up_blocks), dim3(256), 0, c->stream, c->cat.get(), c->pi_tmp.get(), d_pairs, np, d_tab);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    if ((rc = pmx_prof_begin(c, "precise_average|pi_average_kernel", (double)maps_floats * 4))) return rc;
    hipLaunchKernelGGL(pi_average_kernel, dim3((unsigned)dn_blocks), dim3(256), 0, c->stream, c->pi_tmp.get(), c->pi_maps.get(), d_pairs, d_imgs, n, d_tab);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    c->pi_off.assign(n, 0); c->pi_hw.assign(2 * (size_t)n, 0);
    for (int i = 0; i < n; ++i) { c->pi_off[i] = pim[i].out; c->pi_hw[2 * i] = pim[i].oh; c->pi_hw[2 * i + 1] = pim[i].ow; }

    // ---- post-process at the original size (:475-481): img_len = orig_w, no rescale; one launch set per run of equal sizes
    std::vector<PPCall> calls;
    for (int i = 0; i < n; ++i) {
        const int oh = pim[i].oh, ow = pim[i].ow;
        if (!calls.empty() && calls.back().map_h == oh && calls.back().map_w == ow) { calls.back().B += 1; continue; }
        const long long hw = (long long)oh * ow;
        PPCall q{};
        q.maps.paf = c->pi_maps + pim[i].out;
        q.maps.heat = c->pi_maps + pim[i].out + PMX_N_PAF * hw;
        q.maps.sx = 1; q.maps.sy = ow; q.maps.sc = hw;
        q.maps.sbh = q.maps.sbp = PI_CH * hw;
        q.maps.fh = oh; q.maps.fw = ow;
        q.tab = tab_of[std::make_pair(oh, ow)];
        q.base = i; q.B = 1; q.map_h = oh; q.map_w = ow; q.img_len = (double)ow; q.has_scale = false;
        q.limbs_slices = c->opt_limbs_slices >= 0 ? c->opt_limbs_slices : 8;      // (pmx_postprocess on full-resolution maps)
        calls.push_back(q);
    }
    for (const PPCall& q : calls) {
        if ((rc = pmx_prof_begin(c, "postprocess|pp_launch", 0))) return rc;
        if ((rc = pp_launch(q.maps, q.tab, pmx_pp_view(c->pp, q.base), q.B, q.map_h, q.map_w, q.img_len, nullptr, 0, c->opt_pp_generic, c->stream, nullptr, nullptr,
                            q.limbs_slices))) return rc;
        if ((rc = pmx_prof_end(c))) return rc;
    }
    c->pp_calls = calls;
    c->pp_valid = true; c->pp_final = false; c->pp_B = n; c->pp_h = c->pp_w = 0;
    c->pp_has_scale = false;
    return PMX_OK;
}

// the averaged maps of image `image` of the last pmx_detect_precise_images call, NCHW float32 (either pointer may be NULL); synchronises
extern "C" int pmx_get_precise_image_maps(pmx_ctx* c, int image, float* paf, float* heat, int h, int w)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    PMX_CHECK(!c->pi_off.empty(), PMX_ERR_STATE, "pmx_get_precise_image_maps: no pmx_detect_precise_images call yet");
    PMX_CHECK(image >= 0 && image < (int)c->pi_off.size(), PMX_ERR_INVALID, "pmx_get_precise_image_maps: image %d outside 0..%d", image,
              (int)c->pi_off.size() - 1);
    const int oh = c->pi_hw[2 * image], ow = c->pi_hw[2 * image + 1];
    PMX_CHECK(h == oh && w == ow, PMX_ERR_INVALID, "pmx_get_precise_image_maps: image %d has %d x %d maps (asked for %d x %d)", image, oh, ow, h, w);
    PMX_DEV(c);
    const size_t hw = (size_t)oh * ow;
    const float* base = c->pi_maps + c->pi_off[image];
    if (paf) PMX_HIP(hipMemcpyAsync(paf, base, hw * PMX_N_PAF * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (heat) PMX_HIP(hipMemcpyAsync(heat, base + hw * PMX_N_PAF, hw * PMX_N_HEAT * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    PMX_HIP(hipStreamSynchronize(c->stream));
    return PMX_OK;
}

extern "C" int pmx_precise_images_table_bytes(pmx_ctx* c, size_t* bytes)
{
    PMX_CHECK(c && bytes, PMX_ERR_INVALID, "null arg");
    *bytes = c->pi_dev.capacity();
    return PMX_OK;
}
