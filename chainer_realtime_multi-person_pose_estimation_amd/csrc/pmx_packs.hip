// pmx_packs.hip -- the weight packers: the only place a pack of PackedLayer gets built -- direct, f16, bf16x3, transposed, Winograd, conv1_1's
// fused-kernel pack -- and the un-pack back to OIHW.  One thread per element of a pack, `dst[idx] = value(idx)` over the definitions in
// pack_index.h, so the pad positions are written (+0) like everything else.  This unit is compiled with -ffp-contract=off: the Winograd
// transform is a sequence of double multiplies and adds, each rounded (pack_index.h::pmx_pk_wino_value).
//
// A training step makes ONE launch per kind of pack over all updated layers, driven by a table of PackJob on the device: a job owns the
// blocks [blk0, next blk0), 256 elements of its pack each, so no block straddles two layers; a block finds its job by the search the Adam
// kernel uses, through indices that are uniform over the block, so the loads are scalar.  A one-off build (pmx_set_layer, the lazy builders,
// the single-layer entries) passes its single job by value: no table, no allocation, no upload.
#include "pmx_ctx.h"

namespace {

__device__ __forceinline__ PackJob job_of_block(const PackJob* __restrict__ jobs, int njobs)
{
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].blk0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    return jobs[lo];
}

template <int KIND>
__device__ __forceinline__ void pack_block(const PackJob& j)
{
    const unsigned idx = (blockIdx.x - j.blk0) * 256u + threadIdx.x;
    if (idx >= j.total) return;
    float* const f = static_cast<float*>(j.dst);
    uint16_t* const h = static_cast<uint16_t*>(j.dst);
    if (KIND == PMX_PACK_DIRECT) {
        f[idx] = pmx_pk_direct_value(&j, idx);
        if (idx < (unsigned)j.p.cout_pad) j.bias[idx] = pmx_pk_bias_value(&j, idx);
    }
    else if (KIND == PMX_PACK_F16) h[idx] = pmx_pk_f16_value(&j, idx);
    else if (KIND == PMX_PACK_BF16X3) h[idx] = pmx_pk_bf16x3_value(&j, idx);
    else if (KIND == PMX_PACK_TRANSPOSED) f[idx] = pmx_pk_transposed_value(&j, idx);
    else if (KIND == PMX_PACK_WINO) f[idx] = pmx_pk_wino_value(&j, idx);
    else f[idx] = pmx_pk_conv1_value(&j, idx);
}

template <int KIND>
__global__ __launch_bounds__(256) void pack_table_kernel(const PackJob* __restrict__ jobs, int njobs) { pack_block<KIND>(job_of_block(jobs, njobs)); }
template <int KIND>
__global__ __launch_bounds__(256) void pack_one_kernel(PackJob j) { pack_block<KIND>(j); }

__global__ __launch_bounds__(256) void unpack_kernel(const float* __restrict__ dw, const float* __restrict__ db, float* __restrict__ w, PackGeo p, unsigned total)
{
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < total) w[i] = pmx_pk_unpack_value(dw, db, p, i);
}

unsigned blocks256(size_t total) { return (unsigned)((total + 255) / 256); }

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return PMX_OK;
    pmx_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return PMX_ERR_HIP;
}

const char* const kind_name[PMX_PACK_KINDS] = {"pack_direct", "pack_f16", "pack_bf16x3", "pack_transposed", "pack_wino", "pack_conv1"};

size_t direct_floats(const PackedLayer& L) { return (size_t)L.ks * L.ks * L.nch * L.cout_pad * CK; }

}  // namespace

void pmx_layer_geometry(PackedLayer& L, int cout, int cin, int ks, int cin_pad)
{
    L.cout = cout; L.cin = cin; L.ks = ks;
    L.cin_pad = cin_pad; L.cout_pad = pmx_pk_cout_pad(cout); L.nch = cin_pad / CK;
}

PackJob pmx_pack_job_direct(const float* master, const PackedLayer& L, int kind)
{
    PackJob j{};
    j.src = master; j.dst = L.d_w; j.bias = L.d_b;
    j.p = PackGeo{L.cout, L.cin, L.ks * L.ks, kind, L.nch, L.cout_pad};
    j.total = (unsigned)direct_floats(L);
    return j;
}

PackJob pmx_pack_job_transposed(const float* master, int cout, int cin, int ks, int kind, const PackedLayer& P)
{
    PackJob j{};
    j.src = master; j.dst = P.d_w;
    j.p = PackGeo{cout, cin, ks * ks, kind, P.nch, P.cout_pad};
    j.t_cout = P.cout;
    j.total = (unsigned)direct_floats(P);
    return j;
}

PackJob pmx_pack_job_f16(const PackedLayer& L, uint16_t* dst)
{
    PackJob j{};
    j.src = L.d_w; j.dst = dst;
    j.total = (unsigned)direct_floats(L);
    return j;
}

PackJob pmx_pack_job_bf16x3(const PackedLayer& L, uint16_t* dst)
{
    PackJob j{};
    j.src = L.d_w; j.dst = dst; j.p.cout_pad = L.cout_pad;
    j.total = 3 * (unsigned)direct_floats(L);
    return j;
}

PackJob pmx_pack_job_wino(const PackedLayer& L, float* dst)
{
    PackJob j{};
    j.src = L.d_w; j.dst = dst; j.ks = L.ks; j.p.nch = L.nch; j.p.cout_pad = L.cout_pad;
    j.total = (unsigned)((size_t)pmx_pk_wino_planes(L.ks) * (L.cin_pad / 32) * L.cout_pad * 32);
    return j;
}

PackJob pmx_pack_job_conv1(const PackedLayer& L, float* dst)
{
    PackJob j{};
    j.src = L.d_w; j.dst = dst; j.p.cout_pad = L.cout_pad;
    j.total = PMX_PK_CONV1_FLOATS;
    return j;
}

int pmx_pack_launch_table(int kind, const PackJob* d_jobs, int njobs, unsigned blocks, hipStream_t st)
{
    if (kind == PMX_PACK_DIRECT) pack_table_kernel<PMX_PACK_DIRECT><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    else if (kind == PMX_PACK_F16) pack_table_kernel<PMX_PACK_F16><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    else if (kind == PMX_PACK_BF16X3) pack_table_kernel<PMX_PACK_BF16X3><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    else if (kind == PMX_PACK_TRANSPOSED) pack_table_kernel<PMX_PACK_TRANSPOSED><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    else if (kind == PMX_PACK_WINO) pack_table_kernel<PMX_PACK_WINO><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    else pack_table_kernel<PMX_PACK_CONV1><<<blocks, 256, 0, st>>>(d_jobs, njobs);
    return launched(kind_name[kind]);
}

int pmx_pack_launch_one(int kind, const PackJob& job, hipStream_t st)
{
    const unsigned blocks = blocks256(job.total);
    if (kind == PMX_PACK_DIRECT) pack_one_kernel<PMX_PACK_DIRECT><<<blocks, 256, 0, st>>>(job);
    else if (kind == PMX_PACK_F16) pack_one_kernel<PMX_PACK_F16><<<blocks, 256, 0, st>>>(job);
    else if (kind == PMX_PACK_BF16X3) pack_one_kernel<PMX_PACK_BF16X3><<<blocks, 256, 0, st>>>(job);
    else if (kind == PMX_PACK_TRANSPOSED) pack_one_kernel<PMX_PACK_TRANSPOSED><<<blocks, 256, 0, st>>>(job);
    else if (kind == PMX_PACK_WINO) pack_one_kernel<PMX_PACK_WINO><<<blocks, 256, 0, st>>>(job);
    else pack_one_kernel<PMX_PACK_CONV1><<<blocks, 256, 0, st>>>(job);
    return launched(kind_name[kind]);
}

int pmx_unpack_launch(const PackedLayer& L, int kind, float* dst, hipStream_t st)
{
    const size_t total = (size_t)L.cout * L.cin * L.ks * L.ks + L.cout;
    unpack_kernel<<<blocks256(total), 256, 0, st>>>(L.d_w, L.d_b, dst, PackGeo{L.cout, L.cin, L.ks * L.ks, kind, L.nch, L.cout_pad}, (unsigned)total);
    return launched("unpack");
}
