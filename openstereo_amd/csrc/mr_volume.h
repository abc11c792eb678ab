// IGEV++ multi-range cost volumes (igevpp_stereo.py:182-186): what volume.hip (forward) and backward.hip (the three gradient kernels) share.
//
//   gwc[g,d,w] = (1/K) sum_k L[gK+k,w] R[gK+k,w-d]  (w >= d)      V0 = gwc[:, :S]
//   V1[o,d',w] = sum_g sum_j P0[o,g,j] gwc[g,k0 d'+j,w]  (d' < M/k0)     V2: P1, k1, all D planes
//
// Every kernel gives a lane ONE pixel of a 64-pixel tile of one image row and walks along d; the full-range volume exists only as the 8
// group correlations of the current plane in registers.  The features of the other image are shared through a ring in LDS: pixel x lives
// in slot x & 127 of its channel's row, a step of MR_DS planes reads a window of 64 + MR_DS - 1 pixels and the next step's MR_DS new
// pixels are fetched into registers before the step's arithmetic and written to the ring after it.  The slots they overwrite are
// 128 pixels away from their own, outside the step's window (79 + 16 <= 128), so one barrier per step is enough.
// KT = channels per group when they fit in registers (4, 12), 0 = any K: no ring, both features are read from global memory.
// A walk of all D planes by one wave is a serial chain (D = 192: 0.45 ms whatever the map size), so the range is cut into chunks of DCH
// planes (grid.y), at least two steps each, sized on the host for about 4096 workgroups; a chunk starts on a multiple of MR_DS, so no patch straddles two chunks
// and the results do not depend on the chunking.
#pragma once
#include "osa_common.h"
#include <type_traits>
#include <algorithm>

namespace osa {

constexpr int MR_WT = 64, MR_DS = 16, MR_RING = 128, MR_G = 8;

struct MrArgs {
    const float* L; const float* R; const float* P0; const float* P1;
    float* V0; float* V1; float* V2;        // forward: outputs; backward: the three output gradients (read only, any of them may be NULL)
    float* dL; float* dR; float* ws;
    int B, C, H, W, D, S, M, K, nWt;
    int DCH;                                // planes per workgroup of the d-walking kernels (grid.y = chunk; a multiple of MR_DS)
};

// the checks of the three entry points (host; before any launch)
static inline int mr_check(const char* who, bool ptrs, int B, int C, int H, int W, int G, int Co, int D, int S, int M, int k0, int k1, int layout) {
    OSA_REQUIRE(ptrs, "%s: NULL pointer", who);
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && D > 0, "%s: bad dims", who);
    OSA_REQUIRE(G == MR_G && Co == MR_G, "%s: %d groups / %d output channels (supported: 8 groups and 8 output channels)", who, G, Co);
    OSA_REQUIRE(C % G == 0, "%s: C=%d not divisible by groups=%d", who, C, G);
    OSA_REQUIRE((k0 == 2 || k0 == 4) && (k1 == 2 || k1 == 4), "%s: patch sizes k0=%d, k1=%d (supported: 2 and 4)", who, k0, k1);
    OSA_REQUIRE(0 < S && S <= M && M <= D, "%s: ranges must satisfy 0 < s_range <= m_range <= maxdisp, got %d, %d, %d", who, S, M, D);
    OSA_REQUIRE(M % k0 == 0 && D % k1 == 0, "%s: m_range=%d must be divisible by k0=%d and maxdisp=%d by k1=%d", who, M, k0, D, k1);
    OSA_REQUIRE(layout == OSA_NCDHW || layout == OSA_NDHWC, "%s: layout %d (OSA_NCDHW or OSA_NDHWC)", who, layout);
    OSA_REQUIRE((long long)B * H * cdiv(W, MR_WT) <= 0x7fffffffLL && C <= 65535 && (long long)H * W * D < 0x7fffffffLL, "%s: grid too large", who);
    return 0;
}

static inline int mr_chunk(int nblk, int D) {
    const int nch = (int)std::min<long long>(std::max(1, 4096 / std::max(nblk, 1)), cdiv(D, 2 * MR_DS));
    return std::max(2 * MR_DS, D / nch / MR_DS * MR_DS);
}

// ---- the ring of the other image's features -------------------------------------------------------------------------------------------
// pixels [x0, x0 + n) of every channel of one image row -> ring (prologue; all NTHR threads)
template <int CT, int NTHR>
__device__ __forceinline__ void mr_stage(float* ring, const float* Frow, size_t plane, int W, int x0, int n, int tid) {
    for (int it = tid; it < CT * n; it += NTHR) {
        const int c = it / n, x = x0 + (it - c * n);
        ring[c * MR_RING + (x & (MR_RING - 1))] = (x >= 0 && x < W) ? Frow[(size_t)c * plane + x] : 0.f;
    }
}
// the MR_DS pixels from xn of every channel, in two halves around a step's arithmetic: global -> registers, registers -> ring
template <int CT, int NTHR>
__device__ __forceinline__ void mr_fetch(float (&nb)[CT * MR_DS / NTHR], const float* Frow, size_t plane, int W, int xn, int tid) {
#pragma unroll
    for (int i = 0; i < CT * MR_DS / NTHR; ++i) {
        const int it = i * NTHR + tid, c = it / MR_DS, x = xn + (it & (MR_DS - 1));
        nb[i] = (x >= 0 && x < W) ? Frow[(size_t)c * plane + x] : 0.f;
    }
}
template <int CT, int NTHR>
__device__ __forceinline__ void mr_commit(float* ring, const float (&nb)[CT * MR_DS / NTHR], int xn, int tid) {
#pragma unroll
    for (int i = 0; i < CT * MR_DS / NTHR; ++i) {
        const int it = i * NTHR + tid, c = it / MR_DS, x = xn + (it & (MR_DS - 1));
        ring[c * MR_RING + (x & (MR_RING - 1))] = nb[i];
    }
}

// P[o][g][j] (the Conv3d weight [8, 8, k, 1, 1]) -> LDS as [j][g][o]: the 8 output channels of a (j, g) are two float4 broadcasts
template <int KP, int NTHR>
__device__ __forceinline__ void mr_stage_patch(float* Ps, const float* P, int tid) {
    for (int i = tid; i < 64 * KP; i += NTHR) {
        const int o = i / (MR_G * KP), g = (i / KP) % MR_G, j = i % KP;
        Ps[(j * MR_G + g) * MR_G + o] = P[i];
    }
}

// the 8 group correlations of pixel w at disparity d: the k-ordered fmaf chain and the division by K of build_volume_ncdhw_kernel
template <int KT>
__device__ __forceinline__ void mr_gwc(float (&c)[MR_G], const float (&Lr)[KT ? MR_G * KT : 1], const float* ring, const float* Lrow, const float* Rrow,
                                       size_t plane, int K, float Kf, int w, int d, bool live) {
    const bool valid = w >= d;
    const int x = w - d;
#pragma unroll
    for (int g = 0; g < MR_G; ++g) {
        float s = 0.f;
        if constexpr (KT > 0) {
#pragma unroll
            for (int k = 0; k < KT; ++k) s = fmaf(Lr[g * KT + k], ring[(g * KT + k) * MR_RING + (x & (MR_RING - 1))], s);
        } else if (valid && live) {
            for (int k = 0; k < K; ++k) s = fmaf(Lrow[(size_t)(g * K + k) * plane + w], Rrow[(size_t)(g * K + k) * plane + x], s);
        }
        c[g] = valid ? s / Kf : 0.f;
    }
}

// voxel (b, ch, d, h, w) of a [B, 8, Dn, H, W] volume in either memory format
template <bool CL>
__device__ __forceinline__ size_t mr_vox(int b, int ch, int d, int Dn, int h, int H, int w, int W) {
    if constexpr (CL) return ((((size_t)b * Dn + d) * H + h) * W + w) * MR_G + ch;
    else return ((((size_t)b * MR_G + ch) * Dn + d) * H + h) * W + w;
}
template <bool CL>
__device__ __forceinline__ void mr_load8(float (&v)[MR_G], const float* V, int b, int d, int Dn, int h, int H, int w, int W) {
    if constexpr (CL) {
        const float4* s = reinterpret_cast<const float4*>(V + mr_vox<true>(b, 0, d, Dn, h, H, w, W));
        const float4 a = s[0], e = s[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = e.x; v[5] = e.y; v[6] = e.z; v[7] = e.w;
    } else {
#pragma unroll
        for (int o = 0; o < MR_G; ++o) v[o] = V[mr_vox<false>(b, o, d, Dn, h, H, w, W)];
    }
}
template <bool CL>
__device__ __forceinline__ void mr_store8(float* V, const float (&v)[MR_G], int b, int d, int Dn, int h, int H, int w, int W) {
    if constexpr (CL) {
        float* s = V + mr_vox<true>(b, 0, d, Dn, h, H, w, W);
        store16(s, make_float4(v[0], v[1], v[2], v[3]));
        store16(s + 4, make_float4(v[4], v[5], v[6], v[7]));
    } else {
#pragma unroll
        for (int o = 0; o < MR_G; ++o) V[mr_vox<false>(b, o, d, Dn, h, H, w, W)] = v[o];
    }
}

// dispatch on (channels per group, k0, k1, memory format): F is a generic lambda taking four integral constants
template <class F>
static inline void mr_dispatch(int K, int k0, int k1, int layout, F&& f) {
    auto l4 = [&](auto kt, auto a, auto b_) {
        if (layout == OSA_NDHWC) f(kt, a, b_, std::true_type{}); else f(kt, a, b_, std::false_type{});
    };
    auto l3 = [&](auto kt, auto a) {
        if (k1 == 2) l4(kt, a, std::integral_constant<int, 2>{}); else l4(kt, a, std::integral_constant<int, 4>{});
    };
    auto l2 = [&](auto kt) {
        if (k0 == 2) l3(kt, std::integral_constant<int, 2>{}); else l3(kt, std::integral_constant<int, 4>{});
    };
    if (K == 12) l2(std::integral_constant<int, 12>{});
    else if (K == 4) l2(std::integral_constant<int, 4>{});
    else l2(std::integral_constant<int, 0>{});
}

}  // namespace osa
