// pmx_render.hip -- the result images of the reference's programs on the device: draw_person_pose (pose_detector.py:520-553), the
// cv2.addWeighted(img, 0.6, canvas, 0.4, 0) every program ends with, and per person draw_face_keypoints / draw_hand_keypoints /
// cv2.rectangle of demo.py:30-55.  The contract is the package's own host functions (pose_detector._draw_line / _draw_disc /
// draw_person_pose, face_hand_detector.draw_face_keypoints / draw_hand_keypoints, demo.add_weighted / draw_rectangle / render), byte for
// byte; include/pose_mi355x.h (pmx_render) writes it out.  Compiled with -ffp-contract=off: every float64 / float32 product and sum below
// is rounded on its own, as NumPy rounds it.
//
// Every host drawing step assigns a colour to the pixels it covers, one step after the other, so a pixel ends with the colour of the LAST
// primitive that covers it -- within the pose layer (drawn on a copy of the image, then blended) and within the parts layer (drawn opaque
// over the blended canvas) separately.  The host half of this file turns the poses and parts of a call into one table of primitives in
// drawing order (kind, layer, colour, geometry in the host's own numbers, the clipped bounding box the host function computes); the kernel
// asks, per pixel, which primitive of each layer covers it last.
//
//   render_tiles_kernel   ONE launch per call over the 64 x 16 pixel tiles of ALL images (per-image table: addresses, size, first tile,
//                         first primitive).  A block walks its image's primitives in chunks of one per thread, keeps those whose box
//                         meets the tile (wave64 ballot + prefix count: the survivors stay in table order) in LDS, then every pixel
//                         runs over the survivors.  A lane owns one column of the tile, a wave every fourth row: the 3-byte pixels of
//                         a wave's load / store are 192 consecutive bytes.
#include "pmx_ctx.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int RT_W = 64, RT_H = 16, RT_THREADS = 256, RT_WAVES = RT_THREADS / 64, RT_ROWS = RT_H / RT_WAVES;

enum { RK_LINE2 = 0, RK_LINE1 = 1, RK_DISC = 2, RK_RECT = 3 };     // line of thickness 2 (r = 1) | of thickness 1 (r = 0.5) | disc | outline

// one drawing step.  g: line = (x1, y1, dx, dy, L2) of _draw_line, computed on the host in its order (dx = x2 - x1, L2 = dx * dx + dy * dy);
// disc = (cx, cy, radius^2) as integers; rect = (x0, y0, x1, y1) of draw_rectangle as integers.  bb = (xa, ya, xb, yb): the inclusive
// clipped box the host function assigns inside; a step whose box is empty (the functions' early return) is not in the table.
struct RenderPrim {
    double g[5];
    int bb[4];
    uint32_t info;       // kind | layer << 2 (0 pose, 1 parts) | colour << 8 (channel 0 lowest)
    uint32_t pad;
};
static_assert(sizeof(RenderPrim) == 64, "RenderPrim layout");

struct RenderImg {
    const uint8_t* src;
    uint8_t* dst;
    int h, w, tiles_x, tile0, prim0, n_prims;
};

// A shortcut that never changes a result: is the point at (ax, ay) from the segment's first end farther than sqrt(lim2) from the LINE
// through the segment?  cross = ax * dy - ay * dx is |distance to the line| * sqrt(L2).  The segment is no nearer than its line, and
// _draw_line covers a pixel only within sqrt(r * r + 0.25) <= 1.119 of the segment, so with lim2 >= 1.5^2 a "yes" means "not covered"
// as long as the rounding of this test and of _draw_line's own d2 stays below the 0.38 pixels in between: every coordinate that is
// drawn is below 2^30 in magnitude (pmx_render refuses others), so |ax|, |ay| < 2^31 and the distance carries an absolute error below
// 2^-52 * (|ax| + |ay|) < 2^-20 pixels.  L2 == 0 gives cross == 0: never "yes", the full test decides.
__device__ __forceinline__ bool far_from_line(double ax, double ay, double dx, double dy, double L2, double lim2)
{
    const double cross = ax * dy - ay * dx;
    return cross * cross > lim2 * L2;
}

// does step q cover pixel (x, y)?  (x, y) lies inside q.bb
__device__ __forceinline__ bool covers(const RenderPrim& q, int kind, double px, double py)
{
    if (kind == RK_DISC) {
        const double ex = px - q.g[0], ey = py - q.g[1];              // integers: exact, as _draw_disc's integer test
        return ex * ex + ey * ey <= q.g[2];
    }
    if (kind == RK_RECT) return px == q.g[0] || px == q.g[2] || py == q.g[1] || py == q.g[3];
    // _draw_line: t = clip(((xs - x1) * dx + (ys - y1) * dy) / L2, 0, 1) if L2 > 0 else 0; d2 = (xs - (x1 + t * dx)) ** 2 + (ys - (y1 + t * dy)) ** 2
    const double x1 = q.g[0], y1 = q.g[1], dx = q.g[2], dy = q.g[3], L2 = q.g[4];
    const double ax = px - x1, ay = py - y1;
    if (far_from_line(ax, ay, dx, dy, L2, 1.5 * 1.5)) return false;
    double t = 0.0;
    if (L2 > 0) {
        t = (ax * dx + ay * dy) / L2;
        t = t < 0.0 ? 0.0 : t;
        t = t > 1.0 ? 1.0 : t;
    }
    const double ex = px - (x1 + t * dx), ey = py - (y1 + t * dy);
    return ex * ex + ey * ey <= (kind == RK_LINE2 ? 1.25 : 0.5);     // r * r + 0.25
}

// demo.add_weighted(img, 0.6, canvas, 0.4, 0) for one channel: three float32 operations, round half to even, saturate
__device__ __forceinline__ uint32_t blend_u8(uint32_t s, uint32_t c)
{
    float v = __fadd_rn(__fadd_rn(__fmul_rn((float)s, 0.6f), __fmul_rn((float)c, 0.4f)), 0.0f);
    v = rintf(v);
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (uint32_t)v;
}

__global__ __launch_bounds__(RT_THREADS) void render_tiles_kernel(const RenderImg* __restrict__ imgs, int n_images,
                                                                 const RenderPrim* __restrict__ prims, int blend)
{
    __shared__ RenderPrim s_prim[RT_THREADS];
    __shared__ int s_cnt[RT_WAVES];
    // the image of this block: the last one whose first tile is <= blockIdx.x (every image has a tile; tile0 is strictly increasing)
    int lo = 0, hi = n_images - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const RenderImg im = imgs[lo];
    const int t = (int)blockIdx.x - im.tile0;
    const int tx0 = (t % im.tiles_x) * RT_W, ty0 = (t / im.tiles_x) * RT_H;
    if (tx0 >= im.w || ty0 >= im.h) return;                           // (never: the grid is the sum of the images' tiles)
    const int tx1 = min(tx0 + RT_W, im.w) - 1, ty1 = min(ty0 + RT_H, im.h) - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = tx0 + lane;
    const double px = (double)x;
    const bool in_x = x <= tx1;

    uint32_t src[RT_ROWS], pose[RT_ROWS], part[RT_ROWS];
    unsigned has_pose = 0, has_part = 0;
#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) {
        const int y = ty0 + wave + RT_WAVES * r;
        src[r] = pose[r] = part[r] = 0;
        if (in_x && y <= ty1) {
            const uint8_t* p = im.src + ((size_t)y * im.w + x) * 3;
            src[r] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
        }
    }

    for (int p0 = 0; p0 < im.n_prims; p0 += RT_THREADS) {
        // cull: one primitive per thread against the tile, the survivors compacted in table order
        const int i = p0 + (int)threadIdx.x;
        bool keep = false;
        const RenderPrim* g = prims + im.prim0 + i;
        if (i < im.n_prims) keep = g->bb[0] <= tx1 && g->bb[2] >= tx0 && g->bb[1] <= ty1 && g->bb[3] >= ty0;
        // a long segment's box meets many tiles its line stays away from: every pixel of the tile lies within 33 of the tile's centre
        // (half a diagonal is 32.4), so a centre farther than 33 + 1.5 from the line has no covered pixel (far_from_line)
        if (keep && (g->info & 3) <= RK_LINE1)
            keep = !far_from_line(tx0 + 0.5 * (RT_W - 1) - g->g[0], ty0 + 0.5 * (RT_H - 1) - g->g[1], g->g[2], g->g[3], g->g[4], 34.5 * 34.5);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();                                              // (also: the previous chunk's survivors are no longer read)
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < RT_WAVES; ++w) {
            if (w < wave) base += s_cnt[w];
            n += s_cnt[w];
        }
        if (keep) s_prim[base + __popcll(mask & ((1ull << lane) - 1ull))] = *g;
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const RenderPrim& q = s_prim[k];
            if (x < q.bb[0] || x > q.bb[2]) continue;
            const int kind = q.info & 3, layer = (q.info >> 2) & 1;
            const uint32_t colour = q.info >> 8;
#pragma unroll
            for (int r = 0; r < RT_ROWS; ++r) {
                const int y = ty0 + wave + RT_WAVES * r;
                if (y < q.bb[1] || y > q.bb[3]) continue;
                if (!covers(q, kind, px, (double)y)) continue;
                if (layer) { part[r] = colour; has_part |= 1u << r; }
                else { pose[r] = colour; has_pose |= 1u << r; }
            }
        }
        __syncthreads();                                              // s_cnt and s_prim are rewritten by the next chunk
    }

#pragma unroll
    for (int r = 0; r < RT_ROWS; ++r) {
        const int y = ty0 + wave + RT_WAVES * r;
        if (!in_x || y > ty1) continue;
        uint32_t c = (has_pose >> r & 1) ? pose[r] : src[r];
        if (blend)
            c = blend_u8(src[r] & 255, c & 255) | blend_u8(src[r] >> 8 & 255, c >> 8 & 255) << 8 | blend_u8(src[r] >> 16 & 255, c >> 16 & 255) << 16;
        if (has_part >> r & 1) c = part[r];
        uint8_t* p = im.dst + ((size_t)y * im.w + x) * 3;
        p[0] = (uint8_t)c; p[1] = (uint8_t)(c >> 8); p[2] = (uint8_t)(c >> 16);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
// colours of draw_person_pose (pose_detector.py: LIMB_COLORS, JOINT_COLORS), of draw_face_keypoints and of the fingers
// (face_hand_detector.py: FINGER_COLORS), as the host assigns them to channels 0, 1, 2
const int LIMB_COLORS[PMX_N_LIMBS][3] = {
    {0, 255, 0}, {0, 255, 85}, {0, 255, 170}, {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {255, 0, 0}, {255, 85, 0}, {255, 170, 0},
    {255, 255, 0}, {255, 0, 85}, {170, 255, 0}, {85, 255, 0}, {170, 0, 255}, {0, 0, 255}, {0, 0, 255}, {255, 0, 255}, {170, 0, 255},
    {255, 0, 170}};
const int JOINT_COLORS[PMX_N_JOINTS][3] = {
    {255, 0, 0}, {255, 85, 0}, {255, 170, 0}, {255, 255, 0}, {170, 255, 0}, {85, 255, 0}, {0, 255, 0}, {0, 255, 85}, {0, 255, 170},
    {0, 255, 255}, {0, 170, 255}, {0, 85, 255}, {0, 0, 255}, {85, 0, 255}, {170, 0, 255}, {255, 0, 255}, {255, 0, 170}, {255, 0, 85}};
const int FACE_COLOR[3] = {255, 255, 0}, WHITE[3] = {255, 255, 255};
const int FINGER_COLORS[5][3] = {{0, 0, 255}, {0, 255, 255}, {0, 255, 0}, {255, 0, 0}, {255, 0, 255}};
constexpr int FACE_POINTS = 70, HAND_POINTS = 21;
constexpr double COORD_LIMIT = 1073741824.0;      // 2^30: every coordinate that is drawn is smaller in magnitude (int32 boxes, exact float64 integers)

uint32_t pack_info(int kind, int layer, const int* c)
{
    return (uint32_t)kind | (uint32_t)layer << 2 | (uint32_t)c[0] << 8 | (uint32_t)c[1] << 16 | (uint32_t)c[2] << 24;
}

// the primitives of ONE image, appended in drawing order; each method is the host function of its name up to the assignment
struct PrimList {
    std::vector<RenderPrim>* out;
    int h, w;

    void line(double x1, double y1, double x2, double y2, int thickness, int layer, const int* colour)
    {
        const double r = thickness / 2.0;
        const double fxa = std::floor(std::fmin(x1, x2) - r), fxb = std::ceil(std::fmax(x1, x2) + r);
        const double fya = std::floor(std::fmin(y1, y2) - r), fyb = std::ceil(std::fmax(y1, y2) + r);
        const int xa = fxa < 0 ? 0 : (int)fxa, xb = fxb > w - 1 ? w - 1 : (int)fxb;
        const int ya = fya < 0 ? 0 : (int)fya, yb = fyb > h - 1 ? h - 1 : (int)fyb;
        if (xa > xb || ya > yb) return;
        RenderPrim p{};
        const double dx = x2 - x1, dy = y2 - y1;
        p.g[0] = x1; p.g[1] = y1; p.g[2] = dx; p.g[3] = dy; p.g[4] = dx * dx + dy * dy;
        p.bb[0] = xa; p.bb[1] = ya; p.bb[2] = xb; p.bb[3] = yb;
        p.info = pack_info(thickness == 2 ? RK_LINE2 : RK_LINE1, layer, colour);
        out->push_back(p);
    }
    void disc(long long cx, long long cy, int radius, int layer, const int* colour)
    {
        const long long xa = std::max(0ll, cx - radius), xb = std::min((long long)w - 1, cx + radius);
        const long long ya = std::max(0ll, cy - radius), yb = std::min((long long)h - 1, cy + radius);
        if (xa > xb || ya > yb) return;
        RenderPrim p{};
        p.g[0] = (double)cx; p.g[1] = (double)cy; p.g[2] = (double)(radius * radius);
        p.bb[0] = (int)xa; p.bb[1] = (int)ya; p.bb[2] = (int)xb; p.bb[3] = (int)yb;
        p.info = pack_info(RK_DISC, layer, colour);
        out->push_back(p);
    }
    void rect(int px0, int py0, int px1, int py1, int layer, const int* colour)
    {
        const int x0 = std::min(px0, px1), x1 = std::max(px0, px1), y0 = std::min(py0, py1), y1 = std::max(py0, py1);
        const int cx0 = std::max(x0, 0), cx1 = std::min(x1, w - 1), cy0 = std::max(y0, 0), cy1 = std::min(y1, h - 1);
        if (cx0 > cx1 || cy0 > cy1) return;
        RenderPrim p{};
        p.g[0] = x0; p.g[1] = y0; p.g[2] = x1; p.g[3] = y1;
        p.bb[0] = cx0; p.bb[1] = cy0; p.bb[2] = cx1; p.bb[3] = cy1;
        p.info = pack_info(RK_RECT, layer, colour);
        out->push_back(p);
    }
};

bool drawable(double v) { return std::isfinite(v) && std::fabs(v) < COORD_LIMIT; }

// draw_person_pose: np.round (half to even) of everything, limbs of all people (9 and 13 skipped), then the joints of all people
void pose_prims(PrimList& pl, const double* poses, int n)
{
    std::vector<long long> q((size_t)n * PMX_N_JOINTS * 3);
    for (size_t i = 0; i < q.size(); ++i) {
        const double v = std::nearbyint(poses[i]);
        q[i] = drawable(v) ? (long long)v : 1;          // (only v columns can be out of range here: non-zero is all that matters)
    }
    for (int p = 0; p < n; ++p)
        for (int l = 0; l < PMX_N_LIMBS; ++l) {
            if (l == 9 || l == 13) continue;
            const long long *a = &q[((size_t)p * PMX_N_JOINTS + PMX_LIMBS[l][0]) * 3], *b = &q[((size_t)p * PMX_N_JOINTS + PMX_LIMBS[l][1]) * 3];
            if (a[2] != 0 && b[2] != 0) pl.line((double)a[0], (double)a[1], (double)b[0], (double)b[1], 2, 0, LIMB_COLORS[l]);
        }
    for (int p = 0; p < n; ++p)
        for (int j = 0; j < PMX_N_JOINTS; ++j) {
            const long long* a = &q[((size_t)p * PMX_N_JOINTS + j) * 3];
            if (a[2] != 0) pl.disc(a[0], a[1], 3, 0, JOINT_COLORS[j]);
        }
}

// draw_face_keypoints / draw_hand_keypoints + draw_rectangle for one part; kp: rows (x, y, confidence, valid) in the box's frame
void part_prims(PrimList& pl, const pmx_render_part& part, const double* kp)
{
    const double left = (double)part.left, top = (double)part.top;
    auto X = [&](int i) { return kp[4 * i] + left; };
    auto Y = [&](int i) { return kp[4 * i + 1] + top; };
    auto valid = [&](int i) { return kp[4 * i + 3] != 0.0; };
    if (part.kind == 0) {
        for (int i = 0; i < FACE_POINTS; ++i)
            if (valid(i)) pl.disc((long long)X(i), (long long)Y(i), 2, 1, FACE_COLOR);
        // params['face_line_indices'] (entity.py): the open polylines 0-16, 17-21, 22-26, 27-30, 31-35, the closed ones 36-41, 42-47, 48-59, 60-67
        static const int open_runs[5][2] = {{0, 16}, {17, 21}, {22, 26}, {27, 30}, {31, 35}};
        static const int closed_runs[4][2] = {{36, 41}, {42, 47}, {48, 59}, {60, 67}};
        auto seg = [&](int a, int b) { if (valid(a) && valid(b)) pl.line(X(a), Y(a), X(b), Y(b), 1, 1, FACE_COLOR); };
        for (const auto& r : open_runs)
            for (int i = r[0]; i < r[1]; ++i) seg(i, i + 1);
        for (const auto& r : closed_runs)
            for (int i = r[0]; i <= r[1]; ++i) seg(i, i < r[1] ? i + 1 : r[0]);
    } else {
        // params['fingers_indices']: finger f = bones (0 | 4 f + k, 4 f + k + 1), k = 0 .. 3
        for (int f = 0; f < 5; ++f)
            for (int k = 0; k < 4; ++k) {
                const int a = k == 0 ? 0 : 4 * f + k, b = 4 * f + k + 1;
                if (valid(a)) pl.disc((long long)X(a), (long long)Y(a), 3, 1, FINGER_COLORS[f]);
                if (valid(b)) pl.disc((long long)X(b), (long long)Y(b), 3, 1, FINGER_COLORS[f]);
                if (valid(a) && valid(b)) pl.line(X(a), Y(a), X(b), Y(b), 1, 1, FINGER_COLORS[f]);
            }
    }
    pl.rect(part.left, part.top, part.right, part.bottom, 1, WHITE);
}

int part_points(int kind) { return kind == 0 ? FACE_POINTS : HAND_POINTS; }

// everything pmx_render refuses, before anything is enqueued
int check_render(const pmx_box_image* images, int n_images, const double* poses, const int* n_people, const pmx_render_part* parts, int n_parts,
                 const double* keypoints, int blend, const void* out)
{
    PMX_CHECK(n_images >= 0, PMX_ERR_INVALID, "render: n_images = %d", n_images);
    PMX_CHECK(n_parts >= 0, PMX_ERR_INVALID, "render: n_parts = %d", n_parts);
    if (n_images == 0) {
        PMX_CHECK(n_parts == 0, PMX_ERR_INVALID, "render: part 0: image index %d outside an empty image list", parts ? parts[0].image : 0);
        return PMX_OK;
    }
    PMX_CHECK(images && out, PMX_ERR_INVALID, "render: null %s", images ? "output" : "image list");
    for (int k = 0; k < n_images; ++k)
        PMX_CHECK(images[k].bgr && images[k].h >= 1 && images[k].w >= 1, PMX_ERR_INVALID, "render: image %d: %s, %d x %d", k,
                  images[k].bgr ? "bad size" : "null pointer", images[k].h, images[k].w);
    size_t person = 0;
    for (int k = 0; k < n_images && n_people; ++k) {
        PMX_CHECK(n_people[k] >= 0, PMX_ERR_INVALID, "render: image %d: n_people = %d", k, n_people[k]);
        PMX_CHECK(n_people[k] == 0 || poses, PMX_ERR_INVALID, "render: image %d: %d people and a null pose array", k, n_people[k]);
        for (int p = 0; p < n_people[k]; ++p, ++person)
            for (int j = 0; j < PMX_N_JOINTS; ++j) {
                const double* a = poses + (person * PMX_N_JOINTS + j) * 3;
                PMX_CHECK(std::isfinite(a[2]), PMX_ERR_INVALID, "render: image %d, person %d, joint %d: v = %g", k, p, j, a[2]);
                if (std::nearbyint(a[2]) == 0.0) continue;
                PMX_CHECK(drawable(a[0]) && drawable(a[1]), PMX_ERR_INVALID,
                          "render: image %d, person %d, joint %d: (x, y) = (%g, %g) is not finite or not below 2^30 in magnitude", k, p, j, a[0], a[1]);
            }
    }
    PMX_CHECK(n_parts == 0 || blend, PMX_ERR_INVALID, "render: %d parts with blend = 0 (the parts are drawn over the blended canvas only)", n_parts);
    PMX_CHECK(n_parts == 0 || (parts && keypoints), PMX_ERR_INVALID, "render: %d parts and a null %s array", n_parts, parts ? "key-point" : "part");
    const double* kp = keypoints;
    for (int i = 0; i < n_parts; ++i) {
        const pmx_render_part& pt = parts[i];
        PMX_CHECK(pt.image >= 0 && pt.image < n_images, PMX_ERR_INVALID, "render: part %d: image index %d outside 0..%d", i, pt.image, n_images - 1);
        PMX_CHECK(pt.kind == 0 || pt.kind == 1, PMX_ERR_INVALID, "render: part %d: kind %d (0 face, 1 hand)", i, pt.kind);
        for (int j = 0; j < part_points(pt.kind); ++j, kp += 4) {
            if (kp[3] == 0.0) continue;
            PMX_CHECK(drawable(kp[0] + pt.left) && drawable(kp[1] + pt.top), PMX_ERR_INVALID,
                      "render: part %d, key point %d: (x, y) = (%g, %g) is not finite or not below 2^30 in magnitude", i, j, kp[0] + pt.left, kp[1] + pt.top);
        }
    }
    return PMX_OK;
}

}   // namespace

extern "C" int pmx_render(pmx_ctx* c, const pmx_box_image* images, int n_images, int on_device, const double* poses, const int* n_people,
                          const pmx_render_part* parts, int n_parts, const double* keypoints, int blend, uint8_t* out, int out_on_device)
{
    PMX_CHECK(c, PMX_ERR_INVALID, "null ctx");
    int rc;
    if ((rc = check_render(images, n_images, poses, n_people, parts, n_parts, keypoints, blend, out))) return rc;
    if (n_images == 0) return PMX_OK;
    PMX_DEV(c);

    // the tables: per image its primitives in drawing order (pose layer, then the parts in array order), its tiles, its place in the stores
    std::vector<RenderPrim> prims;
    std::vector<RenderImg> tab(n_images);
    std::vector<size_t> in_off(n_images), out_off(n_images);
    std::vector<const double*> part_kp(n_parts);
    {
        const double* kp = keypoints;
        for (int i = 0; i < n_parts; ++i) { part_kp[i] = kp; kp += 4 * (size_t)part_points(parts[i].kind); }
    }
    size_t person = 0, in_total = 0, out_total = 0;
    long long tiles = 0;
    for (int k = 0; k < n_images; ++k) {
        const int h = images[k].h, w = images[k].w, n = n_people ? n_people[k] : 0;
        PrimList pl{&prims, h, w};
        const size_t first = prims.size();
        if (n) pose_prims(pl, poses + person * PMX_N_JOINTS * 3, n);
        person += n;
        for (int i = 0; i < n_parts; ++i)
            if (parts[i].image == k) part_prims(pl, parts[i], part_kp[i]);
        const int tiles_x = (w + RT_W - 1) / RT_W, tiles_y = (h + RT_H - 1) / RT_H;
        PMX_CHECK(prims.size() < (1u << 30) && tiles + (long long)tiles_x * tiles_y < (1ll << 31), PMX_ERR_CAPACITY,
                  "render: image %d: more than 2^30 primitives or 2^31 tiles in one call", k);
        tab[k] = RenderImg{nullptr, nullptr, h, w, tiles_x, (int)tiles, (int)first, (int)(prims.size() - first)};
        tiles += (long long)tiles_x * tiles_y;
        const size_t bytes = (size_t)h * w * 3;
        in_off[k] = in_total; in_total += pmx_align_up(bytes, 256);
        out_off[k] = out_total; out_total += bytes;
    }
    if (!on_device && (rc = c->rd_img.ensure(in_total, c->stream))) return rc;
    if (!out_on_device && (rc = c->rd_out.ensure(out_total, c->stream))) return rc;
    uint8_t* d_out = out_on_device ? out : c->rd_out.get();
    for (int k = 0; k < n_images; ++k) {
        tab[k].src = on_device ? images[k].bgr : c->rd_img + in_off[k];
        tab[k].dst = d_out + out_off[k];
    }

    // ONE staging copy: [image table | primitives]
    const size_t tab_bytes = pmx_align_up(tab.size() * sizeof(RenderImg), 64), prim_bytes = prims.size() * sizeof(RenderPrim);
    const size_t bytes = tab_bytes + prim_bytes;
    char *host, *dev;
    if ((rc = c->rd.begin(bytes, c->stream, &host, &dev))) return rc;
    memcpy(host, tab.data(), tab.size() * sizeof(RenderImg));
    if (prim_bytes) memcpy(host + tab_bytes, prims.data(), prim_bytes);
    if ((rc = c->rd.commit(bytes, c->stream))) return rc;
    if (!on_device)
        for (int k = 0; k < n_images; ++k)
            PMX_HIP(hipMemcpyAsync(c->rd_img + in_off[k], images[k].bgr, (size_t)images[k].h * images[k].w * 3, hipMemcpyHostToDevice, c->stream));

    if ((rc = pmx_prof_begin(c, "render|render_tiles_kernel", (double)out_total * 2))) return rc;
    hipLaunchKernelGGL(render_tiles_kernel, dim3((unsigned)tiles), dim3(RT_THREADS), 0, c->stream,
                       reinterpret_cast<const RenderImg*>(dev), n_images, reinterpret_cast<const RenderPrim*>(dev + tab_bytes), blend ? 1 : 0);
    PMX_HIP(hipGetLastError());
    if ((rc = pmx_prof_end(c))) return rc;
    if (!out_on_device) {
        PMX_HIP(hipMemcpyAsync(out, c->rd_out, out_total, hipMemcpyDeviceToHost, c->stream));
        PMX_HIP(hipStreamSynchronize(c->stream));
    }
    return PMX_OK;
}
