// f16_sat.h -- the device's fp32 -> f16 conversion of the f16 kernels (conv_f16.hip, conv_wgrad_f16.hip): what they stage into LDS is
// f16_round.h::f16_rn_sat of what lies in HBM.
#ifndef PMX_F16_SAT_H
#define PMX_F16_SAT_H

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// saturating round-to-nearest-even fp32 -> f16 of a staged float4 (the clamp first: v_cvt_f16_f32 would turn |v| >= 65520 into inf).  NaN stays
// NaN, as in the host's f16_rn_sat: a clamp alone makes a finite value of it (fmaxf / fminf and v_med3_f32 return a non-NaN operand), so the
// rare float4 that holds one converts those elements again, unclamped.  One v_med3_f32 per element, one unordered compare per pair
__device__ __forceinline__ f16x4 f16_sat4(const float4 v)
{
    f16x4 h = {(_Float16)__builtin_amdgcn_fmed3f(v.x, -65504.f, 65504.f), (_Float16)__builtin_amdgcn_fmed3f(v.y, -65504.f, 65504.f),
               (_Float16)__builtin_amdgcn_fmed3f(v.z, -65504.f, 65504.f), (_Float16)__builtin_amdgcn_fmed3f(v.w, -65504.f, 65504.f)};
    if (__builtin_expect((v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w), 0)) {
        if (v.x != v.x) h.x = (_Float16)v.x;
        if (v.y != v.y) h.y = (_Float16)v.y;
        if (v.z != v.z) h.z = (_Float16)v.z;
        if (v.w != v.w) h.w = (_Float16)v.w;
    }
    return h;
}

#endif
