// pmx_masks.hip -- the ignore masks of the reference's gen_ignore_mask.py (gen_masks, :23-37) on the device: per image the union of the
// annotations' segmentations (`mask_all`) and the part of it the loss ignores (`mask_miss`, the PNG the reference saves), from polygon and
// run-length parts.  The contract is the package's own host functions (coco.py: polygon_crossings / polygon_mask / rle_mask /
// masks_numpy), byte for byte; include/pose_mi355x.h (pmx_coco_masks) writes it out.  Compiled with -ffp-contract=off: every double
// product and sum below is rounded on its own, as C and NumPy round it; fp64 division is correctly rounded.
//
//   masks_kernel   ONE launch per call; a block owns a STRIP of columns of one image (per-image table: size, first block, strip width,
//                  parts).  It keeps four bit planes of strip x (h + 1) bits in LDS, a column's bits in `wp` consecutive words (wp odd:
//                  columns start in different banks): `toggle` (crossing points of the polygon being filled), `ann` (the annotation so
//                  far), `all`, `miss`.  It walks the image's parts in order:
//                    polygon   the contract traces every edge into a dense point list and reads a crossing point off each consecutive
//                              pair whose u differs.  Only pairs whose smaller u is m = 5 c + 2 pass the column test (xd = c), within an
//                              edge u moves by at most one per point, and at the seam of two edges u only differs where x < 0 (below),
//                              so every (edge, column c of the strip) has AT MOST ONE such pair: a lane takes one (edge, column), finds
//                              the pair in closed form (shallow edge) or by bisection over the contract's own u(t) (steep edge) and
//                              toggles bit (c, yd) with an LDS atomicXor -- XOR commutes, lane order does not matter.  A prefix XOR
//                              down each column turns `toggle` into the filled columns, ORed into `ann`.
//                    run-length  the host gives the running sums of the counts; the block bisects for the first run that reaches its
//                              strip, then a lane per 1-run sets the run's bits of the strip in `ann`.
//                  At the end of an annotation `all` and `miss` take `ann` by the class rule; at the end of the image the two planes are
//                  written as bytes, row-major.  No global atomics, nothing synchronises inside the call.
//
// The seam of two edges: an edge's trace starts at its first vertex and ends at its second, so the pair (last point of edge j, first
// point of edge j + 1) has equal u unless a steep edge's end point u = (int)(X + s * t + .5) differs from X.  s * t is within 2^-30 of
// X' - X (|coordinates| <= 5 * 65536 + 1), so the argument lies within 2^-30 of X + .5 and truncates to X for X >= 0; for X < 0 it
// truncates toward zero to X + 1, and then the pair's smaller u is X < 0: its column test fails (xd < 0).  So seams never yield a
// crossing point, nor does a zero-length edge (one point, both its seams as above).
#include "pmx_ctx.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_MAX_STRIP = 32;                  // columns of a block at most
constexpr int MK_LDS_WORDS = 16384;               // 64 KiB: four planes of strip * wp words
constexpr int MK_MAX_SIDE = 16384;
constexpr double MK_COORD_LIMIT = 65536.0;

struct MaskImg {
    int h, w, part0, n_parts;
    int block0, strip, wp, pad;
    unsigned long long out_off;
};
static_assert(sizeof(MaskImg) == 40, "MaskImg layout");

__host__ __device__ inline int mk_wp(int h) { return ((h + 1 + 31) / 32) | 1; }
__host__ __device__ inline int mk_strip(int h) { const int s = MK_LDS_WORDS / (4 * mk_wp(h)); return s < MK_MAX_STRIP ? s : MK_MAX_STRIP; }

// step 1 of the contract
__device__ __forceinline__ int scale5(double x) { return (int)(5.0 * x + .5); }

// the crossing point of (edge (xs, ys) -> (xe, ye), column with m = 5 c + 2), if there is one: its row yd in 0 .. h
__device__ __forceinline__ bool edge_crossing(int xs, int ys, int xe, int ye, int m, int h, int* yd_out)
{
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    int vmin;
    if (dx >= dy) {
        // u = t + xs for t = 0 .. dx (xs <= xe): the pair with u = m, m + 1
        if (dx == 0 || m < xs || m + 1 > xe) return false;
        const double s = (double)(ye - ys) / dx;
        const int t0 = m - xs;
        const int v0 = (int)(ys + s * t0 + .5), v1 = (int)(ys + s * (t0 + 1) + .5);
        vmin = v0 < v1 ? v0 : v1;
    } else {
        // v = t + ys for t = 0 .. dy (ys < ye), u(t) = (int)(xs + s * t + .5): monotone in t, steps of at most one
        const int lo_x = xs < xe ? xs : xe, hi_x = xs < xe ? xe : xs;
        if (m + 1 < lo_x || m > hi_x + 1) return false;
        const double s = (double)(xe - xs) / dy;
        const bool up = xe >= xs;
        auto U = [&](int t) { return (int)(xs + s * t + .5); };
        auto past = [&](int t) { const int u = U(t); return up ? u >= m + 1 : u <= m; };      // has the trace left the pair's first u?
        if (past(0) || !past(dy)) return false;
        int lo = 0, hi = dy;
        while (hi - lo > 1) {
            const int mid = lo + ((hi - lo) >> 1);
            if (past(mid)) hi = mid; else lo = mid;
        }
        const int ua = U(lo), ub = U(hi);
        if (ua == ub || (ub < ua ? ub : ub - 1) != m) return false;
        vmin = lo + ys;
    }
    // xd = (m + .5) / 5 - .5 = c exactly (c + .5 is representable and the division correctly rounded); the caller has 0 <= c <= w - 1
    double yd = ((double)vmin + .5) / 5.0 - .5;
    if (yd < 0) yd = 0; else if (yd > h) yd = h;
    *yd_out = (int)ceil(yd);
    return true;
}

__global__ __launch_bounds__(MK_THREADS) void masks_kernel(const MaskImg* __restrict__ imgs, int n_images, const pmx_mask_part* __restrict__ parts,
                                                          const double* __restrict__ xy, const uint32_t* __restrict__ cum,
                                                          uint8_t* __restrict__ out_miss, uint8_t* __restrict__ out_all)
{
    extern __shared__ uint32_t lds[];
    int lo = 0, hi = n_images - 1;                                    // the image of this block: the last one whose first block is <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const MaskImg im = imgs[lo];
    const int h = im.h, w = im.w, wp = im.wp;
    const int c0 = ((int)blockIdx.x - im.block0) * im.strip;
    if (c0 >= w) return;                                              // (never: the grid is the sum of the images' strips)
    const int ncol = min(im.strip, w - c0);
    const int plane = im.strip * wp;
    uint32_t *toggle = lds, *ann = lds + plane, *all = lds + 2 * plane, *miss = lds + 3 * plane;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < 4 * plane; i += MK_THREADS) lds[i] = 0;
    __syncthreads();

    for (int p = 0; p < im.n_parts; ++p) {
        const pmx_mask_part pt = parts[im.part0 + p];
        if (pt.kind == 0) {
            const int k = pt.len >> 1;
            const double* v = xy + pt.off;
            for (int item = tid; item < k * ncol; item += MK_THREADS) {
                const int e = item / ncol, cl = item - e * ncol, e1 = e + 1 < k ? e + 1 : 0;
                int yd;
                if (edge_crossing(scale5(v[2 * e]), scale5(v[2 * e + 1]), scale5(v[2 * e1]), scale5(v[2 * e1 + 1]), 5 * (c0 + cl) + 2, h, &yd))
                    atomicXor(&toggle[cl * wp + (yd >> 5)], 1u << (yd & 31));
            }
            __syncthreads();
            // fill: bit y of a column = XOR of its toggle bits 0 .. y
            for (int cl = tid; cl < ncol; cl += MK_THREADS) {
                uint32_t carry = 0;
                for (int i = 0; i < wp; ++i) {
                    uint32_t x = toggle[cl * wp + i];
                    x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;
                    x ^= carry;
                    carry = 0u - (x >> 31);
                    ann[cl * wp + i] |= x;
                    toggle[cl * wp + i] = 0;
                }
            }
            __syncthreads();
        } else {
            // runs of 0 and 1 in turn over the index x * h + y; run r covers [cum[r - 1], cum[r]) and holds ones iff r is odd
            const uint32_t* cs = cum + pt.off;
            const uint32_t g0 = (uint32_t)c0 * (uint32_t)h, g1 = g0 + (uint32_t)ncol * (uint32_t)h;
            int a = 0, b = pt.len;                                    // the first run that ends past g0
            while (a < b) {
                const int mid = a + ((b - a) >> 1);
                if (cs[mid] > g0) b = mid; else a = mid + 1;
            }
            for (int r = (a | 1) + 2 * tid; r < pt.len; r += 2 * MK_THREADS) {
                uint32_t s = cs[r - 1], t = cs[r];
                if (s >= g1) break;
                if (s < g0) s = g0;
                if (t > g1) t = g1;
                while (s < t) {
                    const int cl = (int)((s - g0) / (uint32_t)h);
                    const int y0 = (int)(s - g0) - cl * h;
                    const int y1 = min(h, y0 + (int)(t - s));         // bits y0 .. y1 - 1 of column cl
                    for (int wi = y0 >> 5; wi <= (y1 - 1) >> 5; ++wi) {
                        const int b0 = max(y0 - 32 * wi, 0), b1 = min(y1 - 32 * wi, 32);
                        const uint32_t mask = (b1 == 32 ? 0xffffffffu : (1u << b1) - 1u) & ~((1u << b0) - 1u);
                        atomicOr(&ann[cl * wp + wi], mask);
                    }
                    s += (uint32_t)(y1 - y0);
                }
            }
            __syncthreads();
        }
        if (p + 1 == im.n_parts || parts[im.part0 + p + 1].ann != pt.ann) {
            // the class rule, with `all` as it was before this annotation
            for (int i = tid; i < plane; i += MK_THREADS) {
                const uint32_t m = ann[i], al = all[i];
                if (pt.cls == 2) miss[i] |= m & ~al;
                else if (pt.cls == 1) miss[i] |= m;
                all[i] = al | m;
                ann[i] = 0;
            }
            __syncthreads();
        }
    }

    // the planes as bytes, row-major: consecutive lanes write consecutive columns of a row
    for (int i = tid; i < ncol * h; i += MK_THREADS) {
        const int y = i / ncol, cl = i - y * ncol;
        const int word = cl * wp + (y >> 5), bit = y & 31;
        const size_t o = (size_t)im.out_off + (size_t)y * w + (size_t)(c0 + cl);
        if (out_miss) out_miss[o] = (uint8_t)(miss[word] >> bit & 1u);
        if (out_all) out_all[o] = (uint8_t)(all[word] >> bit & 1u);
    }
}

// everything pmx_coco_masks refuses, before anything is enqueued
int check_masks(const pmx_mask_image* images, int n_images, const pmx_mask_part* parts, int n_parts, const double* xy, size_t n_xy,
                const uint32_t* counts, size_t n_counts, const void* mask_miss, const void* mask_all)
{
    PMX_CHECK(images && n_images > 0, PMX_ERR_INVALID, "coco_masks: %s", images ? "n_images <= 0" : "null image table");
    PMX_CHECK(n_parts >= 0 && (n_parts == 0 || parts), PMX_ERR_INVALID, "coco_masks: %d parts and a null part table", n_parts);
    PMX_CHECK(mask_miss || mask_all, PMX_ERR_INVALID, "coco_masks: both outputs are null");
    PMX_CHECK((n_xy == 0 || xy) && (n_counts == 0 || counts), PMX_ERR_INVALID, "coco_masks: null %s array", n_xy && !xy ? "vertex" : "counts");
    for (int k = 0; k < n_images; ++k) {
        const pmx_mask_image& im = images[k];
        PMX_CHECK(im.h >= 1 && im.w >= 1 && im.h <= MK_MAX_SIDE && im.w <= MK_MAX_SIDE, PMX_ERR_INVALID, "coco_masks: image %d: %d x %d (sides 1 .. %d)", k,
                  im.h, im.w, MK_MAX_SIDE);
        PMX_CHECK(im.n_parts >= 0 && im.part0 >= 0 && (long long)im.part0 + im.n_parts <= n_parts, PMX_ERR_INVALID,
                  "coco_masks: image %d: parts %d .. %d outside the table of %d", k, im.part0, im.part0 + im.n_parts - 1, n_parts);
        for (int p = 0; p < im.n_parts; ++p) {
            const pmx_mask_part& pt = parts[im.part0 + p];
            PMX_CHECK(pt.kind == 0 || pt.kind == 1, PMX_ERR_INVALID, "coco_masks: image %d, part %d: kind %d (0 polygon, 1 run-length)", k, p, pt.kind);
            PMX_CHECK(pt.cls >= 0 && pt.cls <= 2, PMX_ERR_INVALID, "coco_masks: image %d, part %d: class %d (0 keep, 1 miss, 2 crowd)", k, p, pt.cls);
            PMX_CHECK(pt.ann >= 0, PMX_ERR_INVALID, "coco_masks: image %d, part %d: annotation index %d", k, p, pt.ann);
            if (p) {
                const pmx_mask_part& pr = parts[im.part0 + p - 1];
                PMX_CHECK(pt.ann >= pr.ann, PMX_ERR_INVALID, "coco_masks: image %d, part %d: annotation %d after %d (the parts of an annotation are consecutive)",
                          k, p, pt.ann, pr.ann);
                PMX_CHECK(pt.ann != pr.ann || pt.cls == pr.cls, PMX_ERR_INVALID, "coco_masks: image %d, part %d: annotation %d with classes %d and %d", k, p, pt.ann,
                          pr.cls, pt.cls);
            }
            const size_t limit = pt.kind == 0 ? n_xy : n_counts;
            PMX_CHECK(pt.off >= 0 && pt.len >= 0 && (size_t)pt.off + (size_t)pt.len <= limit, PMX_ERR_INVALID,
                      "coco_masks: image %d, part %d: elements %d .. +%d outside the array of %zu", k, p, pt.off, pt.len, limit);
            if (pt.kind == 0) {
                PMX_CHECK(pt.len >= 6 && pt.len % 2 == 0, PMX_ERR_INVALID, "coco_masks: image %d, part %d: a polygon of %d numbers (at least 6, an even count)", k,
                          p, pt.len);
                for (int i = 0; i < pt.len; ++i)
                    PMX_CHECK(std::isfinite(xy[pt.off + i]) && std::fabs(xy[pt.off + i]) <= MK_COORD_LIMIT, PMX_ERR_INVALID,
                              "coco_masks: image %d, part %d: coordinate %g is not finite or outside +-65536", k, p, xy[pt.off + i]);
            } else {
                unsigned long long sum = 0;
                for (int i = 0; i < pt.len; ++i) sum += counts[pt.off + i];
                PMX_CHECK(sum == (unsigned long long)im.h * im.w, PMX_ERR_INVALID, "coco_masks: image %d, part %d: counts sum to %llu, the image has %llu pixels", k,
                          p, sum, (unsigned long long)im.h * im.w);
            }
        }
    }
    return PMX_OK;
}

}   // namespace

extern "C" int pmx_coco_masks_strip(int h)
{
    return h >= 1 && h <= MK_MAX_SIDE ? mk_strip(h) : 0;
}

extern "C" int pmx_coco_masks(pmx_ctx* c, const pmx_mask_image* images, int n_images, const pmx_mask_part* parts, int n_parts, const double* xy,
                              size_t n_xy, const uint32_t* counts, size_t n_counts, uint8_t* mask_miss, uint8_t* mask_all, int out_on_device)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    int rc;
    if ((rc = check_masks(images, n_images, parts, n_parts, xy, n_xy, counts, n_counts, mask_miss, mask_all))) return rc;

    // the layout of the ONE staging block [image table | parts | vertices | running sums of the counts]
    const size_t img_off = 0, part_off = pmx_align_up((size_t)n_images * sizeof(MaskImg), 64);
    const size_t xy_off = pmx_align_up(part_off + (size_t)n_parts * sizeof(pmx_mask_part), 64);
    const size_t cum_off = pmx_align_up(xy_off + n_xy * sizeof(double), 64);
    const size_t bytes = pmx_align_up(cum_off + n_counts * sizeof(uint32_t), 64);
    PMX_CHECK(bytes <= PMX_MASKS_TABLE_BYTES, PMX_ERR_CAPACITY, "coco_masks: %zu bytes of tables exceed the budget of %zu", bytes, (size_t)PMX_MASKS_TABLE_BYTES);
    long long blocks = 0;
    size_t out_total = 0;
    int lds_words = 0;
    std::vector<MaskImg> tab(n_images);
    for (int k = 0; k < n_images; ++k) {
        const int h = images[k].h, w = images[k].w, strip = mk_strip(h), wp = mk_wp(h);
        tab[k] = MaskImg{h, w, images[k].part0, images[k].n_parts, (int)blocks, strip, wp, 0, (unsigned long long)out_total};
        blocks += (w + strip - 1) / strip;
        out_total += (size_t)h * w;
        lds_words = std::max(lds_words, 4 * strip * wp);
    }
    PMX_CHECK(blocks < (1ll << 31), PMX_ERR_CAPACITY, "coco_masks: more than 2^31 strips in one call");
    PMX_DEV(c);
    const bool to_host = !out_on_device;
    const size_t n_out = (mask_miss ? 1 : 0) + (mask_all ? 1 : 0);
    if (to_host && (rc = c->mk_out.ensure(out_total * n_out, c->stream))) return rc;
    uint8_t* d_miss = to_host ? (mask_miss ? c->mk_out.get() : nullptr) : mask_miss;
    uint8_t* d_all = to_host ? (mask_all ? c->mk_out + (mask_miss ? out_total : 0) : nullptr) : mask_all;

    char *host, *dev;
    if ((rc = c->mk.begin(bytes, c->stream, &host, &dev))) return rc;
    memcpy(host + img_off, tab.data(), tab.size() * sizeof(MaskImg));
    if (n_parts) memcpy(host + part_off, parts, (size_t)n_parts * sizeof(pmx_mask_part));
    if (n_xy) memcpy(host + xy_off, xy, n_xy * sizeof(double));
    // per run-length part the running sums of its counts (each sum <= h * w <= 2^28: checked)
    uint32_t* cum = reinterpret_cast<uint32_t*>(host + cum_off);
    if (n_counts) memset(cum, 0, n_counts * sizeof(uint32_t));
    for (int k = 0; k < n_images; ++k)
        for (int p = 0; p < images[k].n_parts; ++p) {
            const pmx_mask_part& pt = parts[images[k].part0 + p];
            if (pt.kind != 1) continue;
            uint32_t sum = 0;
            for (int i = 0; i < pt.len; ++i) { sum += counts[pt.off + i]; cum[pt.off + i] = sum; }
        }
    if ((rc = c->mk.commit(bytes, c->stream))) return rc;

    if ((rc = pmx_prof_begin(c, "coco_masks|masks_kernel", (double)out_total * n_out))) return rc;
    hipLaunchKernelGGL(masks_kernel, dim3((unsigned)blocks), dim3(MK_THREADS), (size_t)lds_words * sizeof(uint32_t), c->stream,
                       reinterpret_cast<const MaskImg*>(dev + img_off), n_images, reinterpret_cast<const pmx_mask_part*>(dev + part_off),
                       reinterpret_cast<const double*>(dev + xy_off), reinterpret_cast<const uint32_t*>(dev + cum_off), d_miss, d_all);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    if (to_host) {
        if (mask_miss) PMX_HIP(hipMemcpyAsync(mask_miss, d_miss, out_total, hipMemcpyDeviceToHost, c->stream));
        if (mask_all) PMX_HIP(hipMemcpyAsync(mask_all, d_all, out_total, hipMemcpyDeviceToHost, c->stream));
        PMX_HIP(hipStreamSynchronize(c->stream));
    }
    return PMX_OK;
}
