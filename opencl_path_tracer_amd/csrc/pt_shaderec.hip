// pt_shaderec.hip -- the per-triangle shading records (ShadeRec, pt_internal.hpp) that shade_hit<SK, REC = true> reads.
//   k_shade_records  one thread per packed triangle, run on the context's stream before the first render launch after an upload of
//                    triangles or materials (ensure_shade_records, pt_launch.cpp): the geometric normal as packed, the material's
//                    type, index and kd, and the tangent frame of the cosine lobe for N and for -N.  The frames come from
//                    tangent_frame() itself (pt_device.hpp), the function diffuse_direction is made of, so a record holds the bits
//                    the inline path would compute at every hit; its 1 / sqrt is the same on either side of its wave-level window
//                    (rsqrt_rn, tests/test_gpu_fast_math.py).
#include "pt_device.hpp"

namespace ptamd {

__global__ void __launch_bounds__(256) k_shade_records(const float4* tris, const TriMeta* meta, const pt_material* mats, int n_mats, int n, ShadeRec* out) {
    const int ti = blockIdx.x * blockDim.x + threadIdx.x;
    if (ti >= n) return;
    const float4 c = tris[(size_t)ti * 3 + 2];
    const f3 N = mk(c.y, c.z, c.w);
    const int mati = meta[ti].mati;
    ShadeRec r;
    r.N[0] = N.x;
    r.N[1] = N.y;
    r.N[2] = N.z;
    r.type = kShadeRecNoMaterial;
    r.kd[0] = r.kd[1] = r.kd[2] = 0.0f;
    r.mati = (uint32_t)mati & ~kShadeRecPlain;
    // n_mats = the materials d_mats holds.  pt_upload_materials checks the triangles added so far, but triangles added and uploaded
    // AFTER it are not checked again: a hit on one reads past the array in shade_hit as it always did, but this kernel visits
    // every triangle, hit or not, so it must not follow such an index
    if (mati >= 0 && mati < n_mats) {
        const pt_material* m = &mats[mati];
        r.type = m->type;
        for (int k = 0; k < 3; ++k) r.kd[k] = m->kd.s[k];
        const bool ks_pos0 = __float_as_int(m->ks.s[0]) == 0 && __float_as_int(m->ks.s[1]) == 0 && __float_as_int(m->ks.s[2]) == 0;
        if (m->_pad && ks_pos0) r.mati |= kShadeRecPlain;
    }
    for (int o = 0; o < 2; ++o) {
        f3 Z, X;
        tangent_frame(o == 0 ? N : -N, &Z, &X);
        r.frame[o][0] = Z.x;
        r.frame[o][1] = Z.y;
        r.frame[o][2] = Z.z;
        r.frame[o][3] = X.x;
        r.frame[o][4] = X.y;
        r.frame[o][5] = X.z;
        r.frame[o][6] = 0.0f;
        r.frame[o][7] = 0.0f;
    }
    out[ti] = r;
}

hipError_t launch_shade_records(const float4* tris, const TriMeta* meta, const pt_material* mats, int32_t n_mats, int32_t n, ShadeRec* out, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_shade_records, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tris, meta, mats, (int)n_mats, (int)n, out);
    return hipGetLastError();
}

}  // namespace ptamd
