// Cost-volume constructors for gfx950.
//
// One pass builds the group-wise-correlation part and the concatenation part and
// writes them straight into the (already concatenated) volume buffer, so the
// reference's torch.cat (gwcnet_cost_processor.py:65) never happens.
//
//  * NDHWC (engine layout), three kernels, bit-identical where more than one applies:
//      - d-walking quad lanes (build_volume_walk_kernel): a workgroup owns a pixel tile of one row and walks along d, the right window
//        is an LDS ring refilled by a loader wave through LDS-DMA.  NHWC features, 8-wave tiles; fp32 or split (f16x3) output.  The
//        headline path.
//      - chunked quad lanes (build_volume_quads_kernel): a workgroup owns (pixel tile, disparity chunk) and stages the whole right window
//        of the chunk first.  NHWC or NCHW features.
//      - per channel (build_volume_ndhwc_kernel): lane = output channel; every channel count the quad lanes do not take.
//    The quad-lane kernels share one definition of the lane's role, of its left features, of a voxel quad and of the running maximum.
//    HBM-write bound: 4 B written per 8 FMAs.
//  * NCDHW kernel (reference layout, drop-in functions): lanes run along w, so loads and
//    stores are coalesced rows; operands come from L1/L2.
//  * dormant pair volumes, cat_fms, and the IGEV++ multi-range volumes (mr_volume.h).
// Host side: build_volume_impl validates and chooses; launch_walk / launch_quads / launch_perchannel / launch_ncdhw size and launch.
#include "osa_common.h"
#include <type_traits>

namespace osa {

// ------------------------------------------------------------------ NDHWC ----
struct VolArgs {
    const float* lg; const float* rg; const float* lc; const float* rc;
    float* vol;
    float* meta;           // range block of the volume (meta[0] = running max |value|) or NULL
    int B, C, Cc, H, W, D, G, K;
    int VC, coff;          // volume channel count / first channel written
    int gstride, cstride;  // >0: features are NHWC with this many floats per pixel (engine backbone); 0: NCHW
    int RS;                // LDS row stride (floats per pixel)
    int catbase;           // float offset of the concat channels inside an LDS row
    int nWt, nDch;         // tiles along w, chunks along d
    int mask_left;
};

constexpr int VOL_WT = 16;   // output pixels per tile
constexpr int VOL_DCH = 16;  // disparities per chunk

// Channels [c, c + 4) of pixel (b, h, w) of a feature map with Ct channels.  stride > 0: NHWC with `stride` floats per pixel, one float4;
// stride == 0: NCHW, four plane-strided scalars.  NHWC = true (the walking kernel): the features are NHWC with 16-byte aligned quads by
// eligibility, no run-time test.
typedef float vol_f32x4_t __attribute__((ext_vector_type(4), aligned(4)));   // (concat features promise 4-byte alignment only)
template <bool NHWC = false>
__device__ __forceinline__ float4 load_quad(const float* f, const int stride, const int Ct, const VolArgs& p, const int b, const int h, const int w, const int c) {
    if constexpr (NHWC) return *reinterpret_cast<const float4*>(f + (((size_t)b * p.H + h) * p.W + w) * stride + c);
    if (stride) {
        // (a native vector: as four scalars beside the NCHW form's four, the compiler merges the two forms into stride-selected scalar loads)
        const vol_f32x4_t t = *reinterpret_cast<const vol_f32x4_t*>(f + (((size_t)b * p.H + h) * p.W + w) * stride + c);
        return make_float4(t.x, t.y, t.z, t.w);
    }
    const size_t plane = (size_t)p.H * p.W;
    const float* src = f + ((size_t)b * Ct + c) * plane + (size_t)h * p.W + w;
    return make_float4(src[0], src[plane], src[2 * plane], src[3 * plane]);
}

// running maximum of |value| over a stored quad (by value: with `am` by reference the chunked kernel's d loop loses its remainder form)
__device__ __forceinline__ float amax4(const float am, const float4& o) {
    return fmaxf(am, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
}

template <int QG>  // K/4 : float4s per group
__global__ __launch_bounds__(256) void build_volume_ndhwc_kernel(const VolArgs p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int NPXL = VOL_WT;
    constexpr int NPXR = VOL_WT + VOL_DCH - 1;
    float* Ls = smem;                    // [NPXL][RS]
    float* Rs = smem + NPXL * p.RS;      // [NPXR][RS]

    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int dch = bid % p.nDch; bid /= p.nDch;
    const int wt = bid % p.nWt;   bid /= p.nWt;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int w0 = wt * VOL_WT, d0 = dch * VOL_DCH;
    const int wr0 = w0 - (d0 + VOL_DCH - 1);  // first right pixel of the window

    const int tid = threadIdx.x;
    const size_t plane = (size_t)p.H * p.W;
    const int nq_g = QG * p.G;                     // gwc quads per pixel
    const int nq_c = (p.Cc + 3) >> 2;              // concat quads per pixel
    const int nq = nq_g + nq_c;

    // ---- stage: item = (quad, pixel), pixel fastest -> coalesced global reads along w
    auto stage = [&](float* dst, const float* fg, const float* fc, int npx, int wbase) {
        const int items = nq * npx;
        const bool chan_fast = (p.gstride != 0);   // NHWC: consecutive lanes walk the channel quads of a pixel
        for (int it = tid; it < items; it += 256) {
            int qi, px;
            if (chan_fast) { px = it / nq; qi = it - px * nq; }
            else { qi = it / npx; px = it - qi * npx; }
            const int w = wbase + px;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const bool wok = (w >= 0) && (w < p.W);
            int lpos;
            if (qi < nq_g) {
                const int q = qi / p.G, g = qi - q * p.G;
                lpos = qi * 4;
                if (wok) v = load_quad(fg, p.gstride, p.C, p, b, h, w, g * p.K + q * 4);
            } else {
                // (the last concat quad may be ragged, Cc % 4 != 0: scalars with a count, not load_quad)
                const int qc = qi - nq_g;
                lpos = p.catbase + qc * 4;
                if (wok) {
                    const int rem = p.Cc - qc * 4;
                    const float* src; size_t st;
                    if (p.cstride) { src = fc + (((size_t)b * p.H + h) * p.W + w) * p.cstride + qc * 4; st = 1; }
                    else { src = fc + ((size_t)b * p.Cc + qc * 4) * plane + (size_t)h * p.W + w; st = plane; }
                    v.x = src[0];
                    if (rem > 1) v.y = src[st];
                    if (rem > 2) v.z = src[2 * st];
                    if (rem > 3) v.w = src[3 * st];
                }
            }
            *reinterpret_cast<float4*>(dst + (size_t)px * p.RS + lpos) = v;
        }
    };
    stage(Ls, p.lg, p.lc, NPXL, w0);
    stage(Rs, p.rg, p.rc, NPXR, wr0);
    __syncthreads();

    // ---- compute: lane = output channel, wave = pixel
    const int lane = tid & 63, wave = tid >> 6;
    const int nch = p.G + 2 * p.Cc;
    float am = 0.f;
    const unsigned am_seen = p.meta ? amax_peek(p.meta) : 0u;
    for (int c = lane; c < nch; c += 64) {
        for (int wl = wave; wl < VOL_WT; wl += 4) {
            const int w = w0 + wl;
            if (w >= p.W) break;
            const float* lrow = Ls + wl * p.RS;
            float4 lq[QG];
            float lcat = 0.f;
            int kind;  // 0 gwc, 1 left concat, 2 right concat
            if (c < p.G) {
                kind = 0;
#pragma unroll
                for (int q = 0; q < QG; ++q) lq[q] = *reinterpret_cast<const float4*>(lrow + (q * p.G + c) * 4);
            } else if (c < p.G + p.Cc) {
                kind = 1;
                lcat = lrow[p.catbase + (c - p.G)];
            } else {
                kind = 2;
            }
#pragma unroll 4
            for (int dd = 0; dd < VOL_DCH; ++dd) {
                const int d = d0 + dd;
                if (d >= p.D) break;
                const float* rrow = Rs + (wl + VOL_DCH - 1 - dd) * p.RS;
                float v = 0.f;
                const bool valid = (w >= d);
                if (kind == 0) {
                    if (valid) {
                        float s = 0.f;
#pragma unroll
                        for (int q = 0; q < QG; ++q) {
                            const float4 r = *reinterpret_cast<const float4*>(rrow + (q * p.G + c) * 4);
                            s = fmaf(lq[q].x, r.x, s); s = fmaf(lq[q].y, r.y, s);
                            s = fmaf(lq[q].z, r.z, s); s = fmaf(lq[q].w, r.w, s);
                        }
                        v = s / (float)p.K;
                    }
                } else if (kind == 1) {
                    v = (valid || !p.mask_left) ? lcat : 0.f;
                } else {
                    if (valid) v = rrow[p.catbase + (c - p.G - p.Cc)];
                }
                const size_t vox = (((size_t)b * p.D + d) * p.H + h) * p.W + w;
                p.vol[vox * p.VC + p.coff + c] = v;
                am = fmaxf(am, fabsf(v));
            }
        }
    }
    if (p.meta) publish_amax(p.meta, am, am_seen, smem);
}

// ---- NDHWC, quad lanes: every lane produces 4 consecutive output channels of one voxel ----
// Needs G % 4 == 0, Cc % 4 == 0 and (G + 2Cc) / 4 = NQ a power of two <= 64 (GwcNet: 16).  A wave
// covers 64 / NQ consecutive pixels, so one store instruction writes 64 x 16 B = 1 KB of contiguous
// NDHWC volume (4 voxels for GwcNet) instead of one 256-byte voxel.  The left features of a lane
// (its 4 groups x K channels) live in registers for the whole disparity chunk; only the sliding
// right window goes through LDS, permuted so that the NQ lanes of a voxel read consecutive 16-byte
// slots.  Same k-ordered fmaf chain and the same division by K as the per-channel kernel.
struct VolQArgs {
    VolArgs v;
    int NQ, lgNQ, DCH, RSq;
    // d-walking form, split output (f16x3 chains): the volume is written as a split tensor -- every 16-channel chunk [16 x fp16 hi | 16 x fp16 lo],
    // the bytes of fp32 NDHWC -- scaled by a power of two derived from the FEATURES' range blocks (a bound, known before the first voxel
    // exists: |gwc| <= max|f|^2, |concat| <= max|f_cat|), so that the first aggregation layer stages it by LDS-DMA like every other layer of
    // the chain instead of splitting fp32 values through registers.  split = 0: fp32 output.
    int split;
    const float* gmeta; const float* cmeta;     // range blocks of the gwc / concat feature tensors (left and right images in one tensor)
};

// A lane of the quad-lane kernels: quad cq of the voxel of pixel (wave's first pixel + wsub).
struct QuadLane {
    int cq, wsub, G4;
    int role;              // 0 gwc quad (groups 4 cq .. 4 cq + 3) / 1 left concat quad / 2 right concat quad
    int rq;                // role 2: slot of the quad in a window row
};
template <int QG>
__device__ __forceinline__ QuadLane quad_lane(const VolQArgs& q, const int lane) {
    QuadLane l;
    l.G4 = q.v.G >> 2;
    const int nq_g = QG * q.v.G, nq_c = q.v.Cc >> 2;
    l.cq = lane & (q.NQ - 1); l.wsub = lane >> q.lgNQ;
    l.role = (l.cq < l.G4) ? 0 : ((l.cq < l.G4 + nq_c) ? 1 : 2);
    l.rq = nq_g + (l.cq - l.G4 - nq_c);
    return l;
}

// The lane's left features of pixel w (live: w is inside the map): 4 groups x QG float4s (role 0) or one concat quad (role 1), zeros otherwise.
template <int QG, bool NHWC>
__device__ __forceinline__ void load_left(const VolArgs& p, const QuadLane& l, const int b, const int h, const int w, const bool live,
                                          float4 (&Lr)[4 * QG], float4& lcat) {
    lcat = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4 * QG; ++i) Lr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live && l.role == 0) {
#pragma unroll
        for (int gi = 0; gi < 4; ++gi)
#pragma unroll
            for (int kq = 0; kq < QG; ++kq) Lr[gi * QG + kq] = load_quad<NHWC>(p.lg, p.gstride, p.C, p, b, h, w, (l.cq * 4 + gi) * p.K + kq * 4);
    } else if (live && l.role == 1) {
        lcat = load_quad<NHWC>(p.lc, p.cstride, p.Cc, p, b, h, w, (l.cq - l.G4) * 4);
    }
}

// One output quad from the window row rrow (the right pixel w - d): 4 group means (k-ordered fmaf chains: gi outer, kq inner, x y z w),
// the left concat quad, or the right one.  valid: w >= d.
template <int QG>
__device__ __forceinline__ float4 voxel_quad(const QuadLane& l, const bool valid, const float4 (&Lr)[4 * QG], const float4& lcat,
                                             const float4* win, const size_t row, const int mask_left, const int K) {
    const float4* rrow = win + row;
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l.role == 0) {
        const float Kf = (float)K;
        // mean over K channels: for K a power of two the multiply by 1/K is exact (== the division)
        const bool kpow2 = (K & (K - 1)) == 0;
        const float Kinv = 1.0f / Kf;
        float sv[4];
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) {
            float s = 0.f;
#pragma unroll
            for (int kq = 0; kq < QG; ++kq) {
                const float4 r = rrow[(gi * QG + kq) * l.G4 + l.cq];
                const float4 f = Lr[gi * QG + kq];
                s = fmaf(f.x, r.x, s); s = fmaf(f.y, r.y, s);
                s = fmaf(f.z, r.z, s); s = fmaf(f.w, r.w, s);
            }
            sv[gi] = valid ? (kpow2 ? s * Kinv : s / Kf) : 0.f;
        }
        o = make_float4(sv[0], sv[1], sv[2], sv[3]);
    } else if (l.role == 1) {
        if (valid || !mask_left) o = lcat;
    } else {
        if (valid) o = rrow[l.rq];
    }
    return o;
}

template <int QG, int NWV>     // NWV waves per workgroup (4 or 8): a wider pixel tile amortises the right window
__global__ __launch_bounds__(NWV * 64) void build_volume_quads_kernel(const VolQArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 smq[];
    const VolArgs& p = q.v;
    constexpr int NTHR = NWV * 64;
    const int vpw = 64 >> q.lgNQ, WT = NWV * vpw;
    const int NPXR = WT + q.DCH - 1;

    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int dch = bid % p.nDch; bid /= p.nDch;
    const int wt = bid % p.nWt;   bid /= p.nWt;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int w0 = wt * WT, d0 = dch * q.DCH;
    const int wr0 = w0 - (d0 + q.DCH - 1);            // first right pixel of the window

    const int tid = threadIdx.x;
    const int nq_g = QG * p.G, nq = nq_g + (p.Cc >> 2);

    // ---- this lane's voxel column and role; its left features are requested first so that their
    // latency overlaps the staging of the right window
    const int lane = tid & 63, wave = tid >> 6;
    const QuadLane l = quad_lane<QG>(q, lane);
    const int w = w0 + wave * vpw + l.wsub;
    const bool wlive = w < p.W;
    float4 Lr[4 * QG], lcat;
    load_left<QG, false>(p, l, b, h, w, wlive, Lr, lcat);
    // ---- right window -> LDS.  Source quad (g, kq) goes to slot (g&3)*QG*G4 + kq*G4 + (g>>2).
    // Item = (pixel, quad); the fast index follows the feature layout (NHWC: quads of a pixel, NCHW:
    // pixels of a quad).  A thread walks its items with a carry instead of dividing, and keeps 4
    // loads in flight before the first LDS store.
    {
        const int items = nq * NPXR;
        const bool chan_fast = (p.gstride != 0);
        const int inner = chan_fast ? nq : NPXR;      // extent of the fast index
        const int step_hi = NTHR / inner, step_lo = NTHR - step_hi * inner;
        int hi = tid / inner, lo = tid - hi * inner;
        for (int it0 = tid; it0 < items; it0 += 4 * NTHR) {
            float4 v[4];
            int dst[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qi = chan_fast ? lo : hi, px = chan_fast ? hi : lo;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                dst[u] = -1;
                if (it0 + u * NTHR < items) {
                    const int wr = wr0 + px;
                    const bool wok = (wr >= 0) && (wr < p.W);
                    int pos;
                    if (qi < nq_g) {
                        const int g = qi / QG, kq = qi - g * QG;
                        pos = ((g & 3) * QG + kq) * l.G4 + (g >> 2);
                        if (wok) v[u] = load_quad(p.rg, p.gstride, p.C, p, b, h, wr, g * p.K + kq * 4);
                    } else {
                        pos = qi;
                        if (wok) v[u] = load_quad(p.rc, p.cstride, p.Cc, p, b, h, wr, (qi - nq_g) * 4);
                    }
                    dst[u] = px * q.RSq + pos;
                }
                lo += step_lo; hi += step_hi;
                if (lo >= inner) { lo -= inner; ++hi; }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (dst[u] >= 0) smq[dst[u]] = v[u];
        }
    }

    __syncthreads();

    float* vout = p.vol + p.coff + l.cq * 4;
    float am = 0.f;
    const unsigned am_seen = p.meta ? amax_peek(p.meta) : 0u;
#pragma unroll 4
    for (int dd = 0; dd < q.DCH; ++dd) {
        const int d = d0 + dd;
        if (d >= p.D) break;
        const float4 o = voxel_quad<QG>(l, w >= d, Lr, lcat, smq, (size_t)(wave * vpw + l.wsub + q.DCH - 1 - dd) * q.RSq, p.mask_left, p.K);
        if (wlive) {
            const size_t vox = (((size_t)b * p.D + d) * p.H + h) * p.W + w;
            store16(vout + vox * p.VC, o);
            am = amax4(am, o);
        }
    }
    if (p.meta) publish_amax(p.meta, am, am_seen, reinterpret_cast<float*>(smq));
}

// ---- NDHWC, quad lanes, d-walking form (r4) ----
// The quad-lane kernel above is bound by latency at the occupancy its 70 KB right window allows (2 workgroups per CU): every workgroup
// loads its left features, stages the window, and only then starts to store -- three phases that two workgroups per CU do not overlap
// (ablation in DESIGN.md 3.1: stores 0.05 + staging 0.035 + products 0.02 + launch / left loads / loop 0.05 ms of 0.154).  Here a workgroup
// owns ONE (b, h, 32-pixel tile) and WALKS along d in steps of DS disparities:
//   * the left features of a lane stay in registers for all D disparities (loaded once instead of once per disparity chunk);
//   * the right window is a RING of NB = WT / DS + 2 blocks of DS pixels in LDS (pixel x lives in slot (x - (w0 + 1)) mod (NB * DS)): step
//     s needs the pixels [w0 + 1 - (s + 1) DS, w0 + WT - 1 - s DS] -- DS new pixels on the left per step, which a LOADER WAVE (wave NWV of the
//     workgroup, no other duty) fetches by LDS-DMA (global_load_lds_dwordx4, per-lane source = the permuted quad the slot holds) while the NWV
//     compute waves run the dot products and the stores of step s.  One barrier per step hands the block over (the loader waits for its
//     transfers first; the compute waves never wait on vmcnt, so their stores stay in flight across steps).  The block a transfer
//     overwrites was last read at least one step -- one barrier -- earlier (derivation next to the kernel).
//   * staged bytes per output byte fall from (WT + DCH - 1) / (WT DCH) to (WT + D - 1) / (WT D) pixels per voxel row (0.36 -> 0.26 of the
//     window per output for GwcNet), and there is no second pass over the left features.
// Same lanes, same voxel_quad, same stores as the kernel above: bit-identical output (tests/test_gpu_parity.py).
// NHWC features with 16-byte aligned quads only (the engine's backbone output); everything else keeps the kernel above.
__device__ const float4 g_vol_zeros[64] = {};        // source of the ring slots outside the image / beyond a pixel's quads

// SPLIT: the volume is written as a split tensor (VolQArgs::split; a kernel of its own -- compiled into one kernel behind a run-time branch the
// fp32 loop lost 20 %: 70 -> 92 registers and two unrolled loop bodies, profiles/round4/volume_walk_after_split_support.txt)
template <int QG, int NWV, int DS, bool SPLIT = false>
__global__ __launch_bounds__((NWV + 1) * 64) void build_volume_walk_kernel(const VolQArgs q) {
    extern __shared__ __attribute__((aligned(16))) float4 smq[];
    const VolArgs& p = q.v;
    const int vpw = 64 >> q.lgNQ, WT = NWV * vpw;
    const int NB = WT / DS + 2, NRING = NB * DS;            // ring capacity in pixels (host: WT % DS == 0)
    const int BLKQ = DS * q.RSq;                            // float4 slots per block
    const int NI = (BLKQ + 63) / 64;                        // LDS-DMA instructions per block

    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int wt = bid % p.nWt;   bid /= p.nWt;
    const int h = bid % p.H;
    const int b = bid / p.H;
    const int w0 = wt * WT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G4 = p.G >> 2;
    const int nq_g = QG * p.G, nq_c = p.Cc >> 2, nq = nq_g + nq_c;
    const size_t rowpix = ((size_t)b * p.H + h) * p.W;
    const int nsteps = (p.D + DS - 1) / DS;
    float* const red = reinterpret_cast<float*>(smq + (size_t)NRING * q.RSq);      // publish_amax scratch (NWV + 1 floats) above the ring

    // ---- LDS-DMA instruction i of ring block `blk` <- right pixels [x0, x0 + DS): 64 slots.  Slot j of the block = (pixel j / RSq, position
    // j % RSq); the position -> source quad map is the inverse of the staging permutation of the kernel above.
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smq;
    auto dma_slice = [&](const int blk, const int x0, const int i) {
        const int j = i * 64 + lane;
        const int px = j / q.RSq, pos = j - px * q.RSq;
        const int x = x0 + px;
        const char* src = reinterpret_cast<const char*>(g_vol_zeros) + lane * 16;
        if (j < BLKQ && pos < nq && x >= 0 && x < p.W) {
            if (pos < nq_g) {
                const int a = pos / G4, ghi = pos - a * G4;
                const int g = ghi * 4 + a / QG, kq = a - (a / QG) * QG;
                src = reinterpret_cast<const char*>(p.rg + (rowpix + x) * p.gstride + g * p.K + kq * 4);
            } else src = reinterpret_cast<const char*>(p.rc + (rowpix + x) * p.cstride + (pos - nq_g) * 4);
        }
        const unsigned m0v = __builtin_amdgcn_readfirstlane(smem_lds + (unsigned)((blk * BLKQ + i * 64) * 16));
        if (j < BLKQ) {
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(src), "s"(m0v) : "memory");
        }
    };
    // block index of the pixels [w0 + 1 + k DS, w0 + (k + 1) DS], k may be negative
    auto blk_of = [&](int k) { k %= NB; return k < 0 ? k + NB : k; };
    // a whole ring block by one wave
    auto dma_block = [&](const int blk, const int x0) {
        for (int i = 0; i < NI; ++i) dma_slice(blk, x0, i);
    };

    // ---- prologue: every wave requests its left features (compute waves), then all NWV + 1 waves share the initial window:
    // blocks 0 .. WT / DS - 1 (pixels w0 + 1 .. w0 + WT) and block -1 (step 0's left pixels w0 + 1 - DS .. w0)
    const QuadLane l = quad_lane<QG>(q, lane);
    const bool compute = wave < NWV;
    const int w = w0 + wave * vpw + l.wsub;
    const bool wlive = compute && w < p.W;
    float4 Lr[4 * QG], lcat;
    load_left<QG, true>(p, l, b, h, w, wlive, Lr, lcat);
    {
        const int nbi = WT / DS + 1;                      // blocks of the initial window
        for (int t = wave; t < nbi * NI; t += NWV + 1) {  // (block, instruction) pairs round-robin over the waves
            const int kb = t / NI, i = t - kb * NI;
            const int k = (kb < WT / DS) ? kb : -1;
            dma_slice(blk_of(k), w0 + 1 + k * DS, i);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (also the left features: requested above, needed below)
    __syncthreads();

    float am = 0.f;
    const unsigned am_seen = (p.meta && compute) ? amax_peek(p.meta) : 0u;
    if (!compute) {
        // ================= loader wave: block of step s + 1 while the compute waves run step s =================
        for (int s = 0; s < nsteps; ++s) {
            if (s + 1 < nsteps) dma_block(blk_of(-(s + 2)), w0 + 1 - (s + 2) * DS);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    } else {
        // ================= compute waves =================
        float* vout = p.vol + p.coff + l.cq * 4;
        // split output: scale from the features' ranges (wave-uniform); lanes (cq even, cq + 1) of a voxel pair up -- the even lane stores the
        // 16 bytes of hi halves of both quads, the odd lane the 16 bytes of lo halves (one 16-byte store per lane, as for fp32)
        [[maybe_unused]] float s_out = 1.f;
        if constexpr (SPLIT) {
            const float ag = (p.G > 0 && q.gmeta) ? amax_read(q.gmeta) : 0.f, ac = (p.Cc > 0 && q.cmeta) ? amax_read(q.cmeta) : 0.f;
            s_out = pow2_scale(fmaxf(ag * ag, ac) * 1.0625f);
            if (p.meta && blockIdx.x == 0 && tid == 0) p.meta[1] = s_out;
        }
        const int cch = p.coff + l.cq * 4;                     // first channel of this lane's quad
        [[maybe_unused]] float* const vsplit = p.vol + (cch >> 4) * 16 + ((l.cq & 1) ? 8 : 0) + (((cch & 15) >> 3) * 4);
        int ri = w - (w0 + 1);                                // ring slot of pixel w - d, d = 0 (in [-1, WT - 2])
        if (ri < 0) ri += NRING;
        // (measured and NOT kept: walking the ring offset and the output pointer incrementally instead of recomputing them per disparity --
        // fewer VALU instructions, but a loop-carried chain through the unrolled body: 0.97 -> 1.17 ms at 8 pairs, profiles/round4/volume_walk_incremental_addresses.txt)
        // one disparity of this lane's voxel column
        auto emit = [&](const int d) {
            const float4 o = voxel_quad<QG>(l, w >= d, Lr, lcat, smq, (size_t)ri * q.RSq, p.mask_left, p.K);
            ri = (ri == 0) ? NRING - 1 : ri - 1;
            if constexpr (SPLIT) {
                uint2 h2, l2;
                split_f16(mul4(o, s_out), h2, l2);
                const bool odd = (l.cq & 1) != 0;
                const uint2 send = odd ? h2 : l2;            // what the partner lane stores
                const uint2 recv = make_uint2((unsigned)__builtin_amdgcn_mov_dpp((int)send.x, 0xB1, 0xf, 0xf, true),     // quad_perm [1, 0, 3, 2]
                                              (unsigned)__builtin_amdgcn_mov_dpp((int)send.y, 0xB1, 0xf, 0xf, true));
                if (wlive) {
                    const size_t vox = (((size_t)b * p.D + d) * p.H + h) * p.W + w;
                    store16(vsplit + vox * p.VC, odd ? make_uint4(recv.x, recv.y, l2.x, l2.y) : make_uint4(h2.x, h2.y, recv.x, recv.y));
                    am = amax4(am, o);
                }
            } else if (wlive) {
                const size_t vox = (((size_t)b * p.D + d) * p.H + h) * p.W + w;
                store16(vout + vox * p.VC, o);
                am = amax4(am, o);
            }
        };
        for (int s = 0; s < nsteps; ++s) {
            if constexpr (SPLIT) {
                // (the cross-lane exchange of the split stores is a convergent operation: the unroller will not duplicate it past an early exit,
                // so full steps run a fixed-trip loop and only the last, partial step a counted one)
                const int nd = (p.D - s * DS < DS) ? p.D - s * DS : DS;
                if (nd == DS) {
#pragma unroll 4
                    for (int dd = 0; dd < DS; ++dd) emit(s * DS + dd);
                } else {
                    for (int dd = 0; dd < nd; ++dd) emit(s * DS + dd);
                }
            } else {
#pragma unroll 4
                for (int dd = 0; dd < DS; ++dd) {
                    const int d = s * DS + dd;
                    if (d >= p.D) break;
                    emit(d);
                }
            }
            // step s is read; block s + 1 has landed (the loader waited for it).  s_barrier only: no vmcnt wait, the stores stay in flight
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
    if (p.meta) publish_amax(p.meta, am, am_seen, red);
}

// ------------------------------------------------------------------ NCDHW ----
// One thread per output element, w fastest. grid.y = channel, grid.z = b*D+d.
__global__ __launch_bounds__(256) void build_volume_ncdhw_kernel(const VolArgs p) {
    const int c = blockIdx.y;
    const int bd = blockIdx.z;
    const int b = bd / p.D, d = bd - b * p.D;
    const int hw = blockIdx.x * 256 + threadIdx.x;
    if (hw >= p.H * p.W) return;
    const int h = hw / p.W, w = hw - h * p.W;
    const size_t plane = (size_t)p.H * p.W;
    float v = 0.f;
    const bool valid = (w >= d);
    if (c < p.G) {
        if (valid) {
            const float* l = p.lg + ((size_t)b * p.C + (size_t)c * p.K) * plane + hw;
            const float* r = p.rg + ((size_t)b * p.C + (size_t)c * p.K) * plane + hw - d;
            float s = 0.f;
            for (int k = 0; k < p.K; ++k) s = fmaf(l[k * plane], r[k * plane], s);
            v = s / (float)p.K;
        }
    } else if (c < p.G + p.Cc) {
        if (valid || !p.mask_left) v = p.lc[((size_t)b * p.Cc + (c - p.G)) * plane + hw];
    } else {
        if (valid) v = p.rc[((size_t)b * p.Cc + (c - p.G - p.Cc)) * plane + hw - d];
    }
    p.vol[((((size_t)b * p.VC + p.coff + c) * p.D + d) * plane) + hw] = v;
}

// ------------------------------------------------------------------ dormant variants (cost_volume.py:9-29, 44-56, 108-117) ----
// No shipped config enables them (StereoBase USE_SUB_VOLUME / CoEx-style heads); plain one-thread-per-element kernels, NCDHW like the
// reference, w fastest.  mode 0: CoEx correlation (sum over the channels of a group, D = maxdisp + 1 planes);
// mode 1 / 2: difference volume of compute_volume, side left / right; mode 3: L1 "sub" volume.
struct PairArgs {
    const float* l; const float* r; float* out;
    int B, C, G, H, W, D, mode;
};
__global__ __launch_bounds__(256) void pair_volume_kernel(const PairArgs p) {
    const int oc = blockIdx.y;                              // output channel (group / channel / 0)
    const int bd = blockIdx.z;
    const int b = bd / p.D, d = bd - b * p.D;
    const int hw = blockIdx.x * 256 + threadIdx.x;
    if (hw >= p.H * p.W) return;
    const int w = hw % p.W;
    const size_t plane = (size_t)p.H * p.W;
    const float* lb = p.l + (size_t)b * p.C * plane + hw;
    const float* rb = p.r + (size_t)b * p.C * plane + hw;
    float v = 0.f;
    int OC = 1;
    if (p.mode == 0) {                                      // cost[b,g,d,h,w] = sum_k x[g,k,h,w] * y[g,k,h,w-d]
        OC = p.G;
        const int K = p.C / p.G;
        if (w >= d)
            for (int k = 0; k < K; ++k) v += lb[(size_t)(oc * K + k) * plane] * rb[(size_t)(oc * K + k) * plane - d];   // torch's sum(2): ascending k
    } else if (p.mode == 1) {                               // reference[w] - target[w-d]   (w >= d)
        OC = p.C;
        if (w >= d) v = lb[(size_t)oc * plane] - rb[(size_t)oc * plane - d];
    } else if (p.mode == 2) {                               // target[w+d] - reference[w]   (w < W-d); d = 0: reference - target
        OC = p.C;
        if (d == 0) v = lb[(size_t)oc * plane] - rb[(size_t)oc * plane];
        else if (w < p.W - d) v = rb[(size_t)oc * plane + d] - lb[(size_t)oc * plane];
    } else {                                                // w < d: sum_c |l|;  else: sum_c |l[w] - r[w-d]|
        for (int c = 0; c < p.C; ++c) {
            const float a = lb[(size_t)c * plane];
            v += (w >= d) ? fabsf(a - rb[(size_t)c * plane - d]) : fabsf(a);
        }
    }
    p.out[(((size_t)b * OC + oc) * p.D + d) * plane + hw] = v;
}

// cat_fms with arbitrary (also negative / dilated) disparity samples, psmnet_cost_processor.py:30-47: plane idx holds disparity
// i = disp_index[idx];  i >= 0: columns w >= i get (reference[w], target[w - i]);  i < 0: columns w < W + i get (reference[w], target[w - i]);
// everything else stays zero.
__global__ __launch_bounds__(256) void cat_fms_kernel(const float* __restrict__ ref, const float* __restrict__ tgt, float* __restrict__ out,
                                                      const int* __restrict__ disp_index, int C, int H, int W, int n) {
    const int c2 = blockIdx.y;
    const int b = blockIdx.z / n, idx = blockIdx.z - b * n;
    const int hw = blockIdx.x * 256 + threadIdx.x;
    if (hw >= H * W) return;
    const int w = hw % W, i = disp_index[idx];
    const size_t plane = (size_t)H * W;
    const bool ok = (i >= 0) ? (w >= i) : (w < W + i);
    float v = 0.f;
    if (ok) v = (c2 < C) ? ref[((size_t)b * C + c2) * plane + hw] : tgt[((size_t)b * C + (c2 - C)) * plane + hw - i];
    out[(((size_t)b * 2 * C + c2) * n + idx) * plane + hw] = v;
}

}  // namespace osa

using namespace osa;

extern "C" int osa_cat_fms_f32(const float* reference_fm, const float* target_fm, float* out, const int* disp_index,
                               int B, int C, int H, int W, int n_samples, void* stream) {
    OSA_REQUIRE(reference_fm && target_fm && out && disp_index, "cat_fms: NULL pointer");
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && n_samples > 0, "cat_fms: bad dims");
    OSA_REQUIRE((long long)B * n_samples <= 65535 && 2 * C <= 65535, "cat_fms: grid too large");
    hipLaunchKernelGGL(cat_fms_kernel, dim3(cdiv((long long)H * W, 256), 2 * C, B * n_samples), dim3(256), 0, (hipStream_t)stream,
                       reference_fm, target_fm, out, disp_index, C, H, W, n_samples);
    OSA_LAUNCH_CHECK("cat_fms");
    return 0;
}

extern "C" int osa_pair_volume_f32(const float* left, const float* right, float* out,
                                   int B, int C, int groups, int H, int W, int planes, int mode, void* stream) {
    OSA_REQUIRE(left && right && out, "pair_volume: NULL pointer");
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && planes > 0, "pair_volume: bad dims");
    OSA_REQUIRE(mode >= 0 && mode <= 3, "pair_volume: mode %d (0 coex correlation, 1 / 2 difference left / right, 3 L1 sub volume)", mode);
    if (mode == 0) OSA_REQUIRE(groups > 0 && C % groups == 0, "pair_volume: C=%d not divisible by groups=%d", C, groups);
    PairArgs a{left, right, out, B, C, mode == 0 ? groups : 1, H, W, planes, mode};
    const int oc = (mode == 0) ? groups : ((mode == 3) ? 1 : C);
    OSA_REQUIRE((long long)B * planes <= 65535 && oc <= 65535, "pair_volume: grid too large");
    hipLaunchKernelGGL(pair_volume_kernel, dim3(cdiv((long long)H * W, 256), oc, B * planes), dim3(256), 0, (hipStream_t)stream, a);
    OSA_LAUNCH_CHECK("pair_volume");
    return 0;
}

// ------------------------------------------------------------------ launcher of the fused volume ----
// f(std::integral_constant) of the first of V0, Vs... that equals v, of the last one otherwise (the idiom of mr_dispatch, mr_volume.h)
template <int V0, int... Vs, class F>
static inline void pick(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V0>{});
    else if (v == V0) f(std::integral_constant<int, V0>{});
    else pick<Vs...>(v, f);
}
// launch with `lds` bytes of dynamic LDS; above the default 64 KiB the kernel's limit is raised first
template <class A>
static inline void launch_lds(void (*kernel)(A), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A& a) {
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, a);
}

// d-walking form of the NDHWC builder (build_volume_walk_kernel): disparities per step (4 or 8), 0 = the chunked kernel
static int g_vol_walk_ds = 8;
// ... of the split-output kernel: 4 (72 registers and a 53 KB ring -> 3 workgroups per CU; 84 / 64 KB / 2 at 8).  Measured at 3 pairs per launch,
// the sub-batch of the default line: 0.466-0.506 -> 0.418-0.424 ms, whole model +0.7 % (profiles/round4/volume_walk_step_split.txt); the fp32
// kernel is indifferent at 3 pairs and 2-3 % better with 8 at 8 pairs.
static int g_vol_walk_split_ds = 4;
static long long g_vol_walk_launches = 0;

// the quad-lane kernels' precondition: whole quads of groups and of concat channels, a power of two of them per voxel, 16-byte stores
static bool quads_eligible(int G, int Cc, const float* vol, int vol_channels, int c_off) {
    const int nq4 = (G + 2 * Cc) / 4;
    return (G % 4 == 0) && (Cc % 4 == 0) && nq4 >= 1 && nq4 <= 64 && (nq4 & (nq4 - 1)) == 0 && (vol_channels % 4 == 0) && (c_off % 4 == 0) &&
           (((size_t)vol & 15) == 0);
}
static bool walk_eligible(int G, int K, int Cc, int gwc_stride, int cat_stride, const float* left_cat, const float* right_cat,
                          const float* vol, int vol_channels, int c_off, int W, int maxdisp, int ds) {
    if (!(G == 0 || (K % 4 == 0 && K / 4 <= 4))) return false;
    if (!quads_eligible(G, Cc, vol, vol_channels, c_off)) return false;
    const int WT = 8 * (64 / ((G + 2 * Cc) / 4));
    if (W < 2 * WT) return false;                                   // 8-wave pixel tiles
    if (!(G == 0 || gwc_stride > 0)) return false;
    if (!(Cc == 0 || (cat_stride > 0 && cat_stride % 4 == 0 && ((size_t)left_cat & 15) == 0 && ((size_t)right_cat & 15) == 0))) return false;
    return ds > 0 && WT % ds == 0 && maxdisp > ds;
}

static int launch_walk(VolQArgs qa, int DS, hipStream_t st) {
    VolArgs& a = qa.v;
    const int WT = 8 * (64 / qa.NQ);
    a.nWt = cdiv(a.W, WT); a.nDch = 1;
    qa.DCH = DS;
    const size_t wlds = (size_t)(WT / DS + 2) * DS * qa.RSq * 16 + 64;
    const long long wblk = (long long)a.B * a.H * a.nWt;
    OSA_REQUIRE(wlds <= 160 * 1024 && wblk < (1ll << 31), "build_volume: walk form does not fit (%zu B of LDS)", wlds);
    pick<1, 2, 3, 4>(a.G > 0 ? a.K / 4 : 1, [&](auto qg) {
        pick<4, 8>(DS, [&](auto ds) {
            pick<1, 0>(qa.split ? 1 : 0, [&](auto sp) {
                launch_lds(build_volume_walk_kernel<decltype(qg)::value, 8, decltype(ds)::value, decltype(sp)::value != 0>,
                           dim3((unsigned)wblk), dim3(9 * 64), wlds, st, qa);
            });
        });
    });
    OSA_LAUNCH_CHECK("build_volume_walk");
    ++g_vol_walk_launches;
    return 0;
}

// chunk plan of the chunked quad-lane kernel: D split evenly into the fewest chunks whose right window fits ~52 KiB of LDS (3 workgroups
// of 4 waves per CU; 78 KiB for 2 of 8 waves); very wide feature vectors may use up to the whole 160 KiB.  Fills DCH, nWt, nDch.
static int plan_quads(VolQArgs& qa, int nwv, size_t* lds) {
    VolArgs& a = qa.v;
    const int WT = nwv * (64 / qa.NQ);
    const size_t budget = (nwv == 8) ? 78 * 1024 : 52 * 1024;
    int nchunk = 1;
    while (nchunk < a.D && (size_t)(WT + cdiv(a.D, nchunk) - 1) * qa.RSq * 16 > budget) ++nchunk;
    qa.DCH = cdiv(a.D, nchunk);
    a.nWt = cdiv(a.W, WT); a.nDch = cdiv(a.D, qa.DCH);
    *lds = (size_t)(WT + qa.DCH - 1) * qa.RSq * 16;
    OSA_REQUIRE(*lds <= 160 * 1024, "build_volume: %zu B of LDS needed (> 160 KiB); too many channels", *lds);
    OSA_REQUIRE((long long)a.B * a.H * a.nWt * a.nDch < (1ll << 31), "build_volume: grid too large");
    return 0;
}
static int launch_quads(const VolQArgs& qa, int nwv, size_t lds, hipStream_t st) {
    const VolArgs& a = qa.v;
    const dim3 grid((unsigned)((long long)a.B * a.H * a.nWt * a.nDch)), block(nwv * 64);
    pick<1, 2, 3, 4>(a.G > 0 ? a.K / 4 : 1, [&](auto qg) {
        pick<8, 4>(nwv, [&](auto nw) {
            launch_lds(build_volume_quads_kernel<decltype(qg)::value, decltype(nw)::value>, grid, block, lds, st, qa);
        });
    });
    OSA_LAUNCH_CHECK("build_volume_quads");
    return 0;
}

static int launch_perchannel(VolArgs a, hipStream_t st) {
    const int QG = (a.G > 0) ? a.K / 4 : 1;
    const int gfl = (a.G > 0) ? QG * a.G * 4 : 0;
    a.catbase = gfl;
    int rs = gfl + ((a.Cc + 3) / 4) * 4;
    if (((rs / 4) & 1) == 0) rs += 4;   // row stride / 16B odd -> conflict-free ds_write_b128 staging
    a.RS = rs;
    a.nWt = cdiv(a.W, VOL_WT); a.nDch = cdiv(a.D, VOL_DCH);
    const size_t lds = (size_t)(VOL_WT + VOL_WT + VOL_DCH - 1) * rs * sizeof(float);
    OSA_REQUIRE(lds <= 160 * 1024, "build_volume: %zu B of LDS needed (> 160 KiB); too many channels", lds);
    const long long nblk = (long long)a.B * a.H * a.nWt * a.nDch;
    OSA_REQUIRE(nblk < (1ll << 31), "build_volume: grid too large");
    pick<1, 2, 3, 4>(QG, [&](auto qg) {
        launch_lds(build_volume_ndhwc_kernel<decltype(qg)::value>, dim3((unsigned)nblk), dim3(256), lds, st, a);
    });
    OSA_LAUNCH_CHECK("build_volume_ndhwc");
    return 0;
}

static int launch_ncdhw(const VolArgs& a, hipStream_t st) {
    const int nch = a.G + 2 * a.Cc;
    OSA_REQUIRE((long long)a.B * a.D <= 65535 && nch <= 65535, "build_volume: grid too large");
    dim3 grid(cdiv((long long)a.H * a.W, 256), nch, a.B * a.D), block(256);
    hipLaunchKernelGGL(build_volume_ncdhw_kernel, grid, block, 0, st, a);
    OSA_LAUNCH_CHECK("build_volume_ncdhw");
    return 0;
}

// Validates the arguments, fills the kernels' argument struct and chooses the kernel.  gwc_stride / cat_stride: 0 = NCHW features.
// split != 0: the volume as a split tensor (osa_build_volume_nhwc_split_f16x3), scale from the features' range blocks gwc_meta / cat_meta.
static int build_volume_impl(const float* left_gwc, const float* right_gwc, int C, int num_groups, int gwc_stride,
                             const float* left_cat, const float* right_cat, int Cc, int cat_stride,
                             float* vol, int layout, int vol_channels, int c_off,
                             int B, int H, int W, int maxdisp, int mask_left_concat, void* stream, float* vol_meta,
                             int split, const float* gwc_meta, const float* cat_meta) {
    OSA_REQUIRE(vol != nullptr, "build_volume: vol is NULL");
    OSA_REQUIRE(B > 0 && H > 0 && W > 0 && maxdisp > 0, "build_volume: bad dims B=%d H=%d W=%d D=%d", B, H, W, maxdisp);
    OSA_REQUIRE(C >= 0 && Cc >= 0 && (C > 0 || Cc > 0), "build_volume: nothing to build (C=%d Cc=%d)", C, Cc);
    int G = 0, K = 0;
    if (C > 0) {
        OSA_REQUIRE(left_gwc && right_gwc, "build_volume: gwc features NULL");
        OSA_REQUIRE(num_groups > 0 && C % num_groups == 0,
                    "build_volume: C=%d not divisible by num_groups=%d", C, num_groups);  // cost_volume.py:61
        G = num_groups; K = C / G;
    }
    if (Cc > 0) OSA_REQUIRE(left_cat && right_cat, "build_volume: concat features NULL");
    const int nch = G + 2 * Cc;
    OSA_REQUIRE(c_off >= 0 && c_off + nch <= vol_channels,
                "build_volume: channels [%d,%d) exceed vol_channels=%d", c_off, c_off + nch, vol_channels);
    OSA_REQUIRE(layout == OSA_NCDHW || layout == OSA_NDHWC, "build_volume: bad layout %d", layout);
    hipStream_t st = (hipStream_t)stream;

    VolQArgs qa{};
    VolArgs& a = qa.v;
    a.lg = left_gwc; a.rg = right_gwc; a.lc = left_cat; a.rc = right_cat; a.vol = vol; a.meta = vol_meta;
    a.B = B; a.C = C; a.Cc = Cc; a.H = H; a.W = W; a.D = maxdisp; a.G = G; a.K = K;
    a.VC = vol_channels; a.coff = c_off; a.mask_left = mask_left_concat;
    a.gstride = gwc_stride; a.cstride = cat_stride;
    qa.split = split; qa.gmeta = gwc_meta; qa.cmeta = cat_meta;

    if (layout == OSA_NCDHW) {
        OSA_REQUIRE(gwc_stride == 0 && cat_stride == 0, "build_volume: NHWC features need the NDHWC volume layout and K %% 4 == 0");
        return launch_ncdhw(a, st);
    }
    if (!(G == 0 || (K % 4 == 0 && K / 4 <= 4))) {
        set_error("build_volume: NDHWC layout needs channels-per-group in {4,8,12,16} (got K=%d); "
                  "build NCDHW and convert with osa_ncdhw_to_ndhwc_f32", K);
        return -1;
    }
    if (!quads_eligible(G, Cc, vol, vol_channels, c_off) || exp_set("OSA_VOL_PERCHANNEL")) {
        OSA_REQUIRE(!split, "build_volume: split output needs the quad-lane d-walking form (osa_build_volume_nhwc_split_eligible)");
        return launch_perchannel(a, st);
    }
    const int nq4 = nch / 4;
    qa.NQ = nq4; qa.lgNQ = 0;
    while ((1 << qa.lgNQ) < nq4) ++qa.lgNQ;
    qa.RSq = ((G > 0) ? (K / 4) * G : 0) + Cc / 4;
    if (qa.RSq % 16 > 6) qa.RSq += 16 - qa.RSq % 16;     // keeps the lanes of two neighbouring voxels on distinct 16-byte slots
    // 8 waves per workgroup when the map is wide enough (amortises the right window over 2x the pixels)
    const int nwv = (W >= 8 * (64 / nq4) * 2) ? 8 : 4;
    size_t lds;
    if (int rc = plan_quads(qa, nwv, &lds)) return rc;
    // d-walking form (build_volume_walk_kernel): NHWC features with 16-byte aligned quads, 8-wave pixel tiles
    const int walk_ds = split ? g_vol_walk_split_ds : g_vol_walk_ds;
    const bool walk = walk_eligible(G, K, Cc, gwc_stride, cat_stride, left_cat, right_cat, vol, vol_channels, c_off, W, maxdisp, walk_ds);
    OSA_REQUIRE(!split || (walk && vol_channels % 16 == 0 && c_off % 16 == 0 && nch % 16 == 0),
                "build_volume: split output needs the d-walking form and 16-channel aligned volume channels (osa_build_volume_nhwc_split_eligible)");
    return walk ? launch_walk(qa, walk_ds, st) : launch_quads(qa, nwv, lds, st);
}

extern "C" int osa_volume_walk_step(int ds) {
    const int prev = g_vol_walk_ds;
    if (ds == 0 || ds == 4 || ds == 8) { g_vol_walk_ds = ds; g_vol_walk_split_ds = ds ? ds : 4; }     // (0: the fp32 output falls back to the chunked kernel; the split form exists as a walk only)
    return prev;
}
extern "C" long long osa_volume_walk_launches(void) { return g_vol_walk_launches; }

extern "C" int osa_build_volume_f32(const float* left_gwc, const float* right_gwc, int C, int num_groups,
                                    const float* left_cat, const float* right_cat, int Cc,
                                    float* vol, int layout, int vol_channels, int c_off,
                                    int B, int H, int W, int maxdisp, int mask_left_concat,
                                    float* vol_meta, void* stream) {
    return build_volume_impl(left_gwc, right_gwc, C, num_groups, 0, left_cat, right_cat, Cc, 0, vol, layout,
                             vol_channels, c_off, B, H, W, maxdisp, mask_left_concat, stream, vol_meta, 0, nullptr, nullptr);
}

// what the two NHWC entry points ask of their features; `who` is the prefix of the messages
static int check_nhwc_features(const char* who, const float* left_gwc, const float* right_gwc, int C, int num_groups, int gwc_stride,
                               int Cc, int cat_stride) {
    OSA_REQUIRE((C == 0 || (gwc_stride >= C && gwc_stride % 4 == 0 && ((size_t)left_gwc & 15) == 0 && ((size_t)right_gwc & 15) == 0)),
                "%s: gwc features need stride >= C, stride %% 4 == 0 and 16-byte alignment", who);
    OSA_REQUIRE((Cc == 0 || cat_stride >= Cc), "%s: concat stride %d < Cc %d", who, cat_stride, Cc);
    OSA_REQUIRE(C == 0 || (C / (num_groups > 0 ? num_groups : 1)) % 4 == 0, "%s: channels per group must be a multiple of 4", who);
    return 0;
}

extern "C" int osa_build_volume_nhwc_f32(const float* left_gwc, const float* right_gwc, int C, int num_groups, int gwc_stride,
                                         const float* left_cat, const float* right_cat, int Cc, int cat_stride,
                                         float* vol, int vol_channels, int c_off,
                                         int B, int H, int W, int maxdisp, int mask_left_concat, float* vol_meta, void* stream) {
    if (int rc = check_nhwc_features("build_volume_nhwc", left_gwc, right_gwc, C, num_groups, gwc_stride, Cc, cat_stride)) return rc;
    return build_volume_impl(left_gwc, right_gwc, C, num_groups, gwc_stride ? gwc_stride : C, left_cat, right_cat, Cc,
                             cat_stride ? cat_stride : Cc, vol, OSA_NDHWC, vol_channels, c_off, B, H, W, maxdisp,
                             mask_left_concat, stream, vol_meta, 0, nullptr, nullptr);
}

extern "C" int osa_build_volume_nhwc_split_eligible(const float* left_cat, const float* right_cat, const float* vol, int C, int num_groups,
                                                    int gwc_stride, int Cc, int cat_stride, int vol_channels, int c_off, int W, int maxdisp) {
    const int G = (C > 0) ? num_groups : 0;
    if (C > 0 && (num_groups <= 0 || C % num_groups)) return 0;
    const int K = G ? C / G : 0;
    if (vol_channels % 16 || c_off % 16 || (G + 2 * Cc) % 16) return 0;
    return walk_eligible(G, K, Cc, gwc_stride ? gwc_stride : C, cat_stride ? cat_stride : Cc, left_cat, right_cat, vol, vol_channels, c_off, W, maxdisp,
                         g_vol_walk_split_ds) ? 1 : 0;
}

extern "C" int osa_build_volume_nhwc_split_f16x3(const float* left_gwc, const float* right_gwc, int C, int num_groups, int gwc_stride,
                                                 const float* left_cat, const float* right_cat, int Cc, int cat_stride,
                                                 float* vol, int vol_channels, int c_off,
                                                 int B, int H, int W, int maxdisp, int mask_left_concat,
                                                 const float* gwc_meta, const float* cat_meta, float* vol_meta, void* stream) {
    OSA_REQUIRE(vol_meta != nullptr && (C == 0 || gwc_meta != nullptr) && (Cc == 0 || cat_meta != nullptr),
                "build_volume_nhwc_split: the range blocks of the features and of the volume are required (the scale of the split halves is derived from them)");
    if (int rc = check_nhwc_features("build_volume_nhwc_split", left_gwc, right_gwc, C, num_groups, gwc_stride, Cc, cat_stride)) return rc;
    return build_volume_impl(left_gwc, right_gwc, C, num_groups, gwc_stride ? gwc_stride : C, left_cat, right_cat, Cc,
                             cat_stride ? cat_stride : Cc, vol, OSA_NDHWC, vol_channels, c_off, B, H, W, maxdisp,
                             mask_left_concat, stream, vol_meta, 1, gwc_meta, cat_meta);
}

extern "C" int osa_corr_volume_f32(const float* left, const float* right, float* vol,
                                   int B, int C, int H, int W, int maxdisp, void* stream) {
    // correlation layer == one group over all channels, volume [B,1,D,H,W] == [B,D,H,W]
    return osa_build_volume_f32(left, right, C, 1, nullptr, nullptr, 0, vol, OSA_NCDHW, 1, 0,
                                B, H, W, maxdisp, 1, nullptr, stream);
}

// ------------------------------------------------------------------ IGEV++ multi-range volumes (mr_volume.h) ----
// One launch writes V0, V1 and V2.  A workgroup is 64 pixels of one row and a chunk of planes; its four waves share the right window in the
// LDS ring and take the aligned groups of 4 planes of a step in turn (wave v: (d / 4) % 4 == v; a patch of 2 or 4 planes lies inside one
// group, so a wave's patch sums are complete), each with the lane's left features in registers.  Per plane the lane forms the 8 group correlations once, stores them while d < S and folds them into
// the running patch sums, which leave every k0 / k1 planes.  CL: NDHWC stores (32 bytes per voxel), else the reference's NCDHW.
#include "mr_volume.h"
namespace osa {

template <int KT, int K0, int K1, bool CL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mr_volume_fwd_kernel(const MrArgs p) {
    constexpr int CT = MR_G * KT;
    __shared__ float ring[KT ? CT * MR_RING : 1];
    __shared__ __attribute__((aligned(16))) float Ps0[64 * K0];
    __shared__ __attribute__((aligned(16))) float Ps1[64 * K1];
    unsigned bid = blockIdx.x;
    const int wt = bid % p.nWt; bid /= p.nWt;
    const int h = bid % p.H, b = bid / p.H;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, w0 = wt * MR_WT, w = w0 + lane;
    const bool live = w < p.W;
    const size_t plane = (size_t)p.H * p.W;
    const float* Lrow = p.L + (size_t)b * p.C * plane + (size_t)h * p.W;
    const float* Rrow = p.R + (size_t)b * p.C * plane + (size_t)h * p.W;
    const float Kf = (float)p.K;
    const int D1 = p.M / K0, D2 = p.D / K1;

    const int d0 = blockIdx.y * p.DCH, dend = min(p.D, d0 + p.DCH);
    if (d0 > w0 + MR_WT - 1) {                              // no pixel of the tile reaches this chunk: zeros
        const float z[MR_G] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (live)
            for (int d = d0; d < dend; ++d) {
                if (((d >> 2) & 3) != wv) continue;
                if (d < p.S) mr_store8<CL>(p.V0, z, b, d, p.S, h, p.H, w, p.W);
                if (d < p.M && d % K0 == K0 - 1) mr_store8<CL>(p.V1, z, b, d / K0, D1, h, p.H, w, p.W);
                if (d % K1 == K1 - 1) mr_store8<CL>(p.V2, z, b, d / K1, D2, h, p.H, w, p.W);
            }
        return;
    }
    mr_stage_patch<K0, 256>(Ps0, p.P0, tid);
    mr_stage_patch<K1, 256>(Ps1, p.P1, tid);
    float Lr[KT ? CT : 1];
    if constexpr (KT > 0) {
#pragma unroll
        for (int c = 0; c < CT; ++c) Lr[c] = live ? Lrow[(size_t)c * plane + w] : 0.f;
        mr_stage<CT, 256>(ring, Rrow, plane, p.W, w0 - d0 - MR_DS + 1, MR_WT + MR_DS - 1, tid);
    }
    __syncthreads();

    float a1[MR_G], a2[MR_G];
#pragma unroll
    for (int o = 0; o < MR_G; ++o) a1[o] = a2[o] = 0.f;
    // one patch tap: acc[o] += P[o][g][j] * c[g], g ascending
    auto fold = [&](float (&acc)[MR_G], const float* Ps, const int j, const float (&c)[MR_G]) {
#pragma unroll
        for (int g = 0; g < MR_G; ++g) {
            // (j = d % k at run time: with compile-time taps the compiler hoists all 384 loop-invariant weights into registers)
            const float4 pa = *reinterpret_cast<const float4*>(Ps + (j * MR_G + g) * MR_G), pb = *reinterpret_cast<const float4*>(Ps + (j * MR_G + g) * MR_G + 4);
            acc[0] = fmaf(pa.x, c[g], acc[0]); acc[1] = fmaf(pa.y, c[g], acc[1]); acc[2] = fmaf(pa.z, c[g], acc[2]); acc[3] = fmaf(pa.w, c[g], acc[3]);
            acc[4] = fmaf(pb.x, c[g], acc[4]); acc[5] = fmaf(pb.y, c[g], acc[5]); acc[6] = fmaf(pb.z, c[g], acc[6]); acc[7] = fmaf(pb.w, c[g], acc[7]);
        }
    };
    for (int ds = d0; ds < dend; ds += MR_DS) {
        [[maybe_unused]] float nb[KT ? CT * MR_DS / 256 : 1];
        const int xn = w0 + 1 - ds - 2 * MR_DS;                    // first pixel of the next step's new block
        const bool more = ds + MR_DS < dend;
        if constexpr (KT > 0) if (more) mr_fetch<CT, 256>(nb, Rrow, plane, p.W, xn, tid);
#pragma unroll 1
        for (int d = ds + 4 * wv; d < min(ds + 4 * wv + 4, dend); ++d) {
            float c[MR_G];
            mr_gwc<KT>(c, Lr, ring, Lrow, Rrow, plane, p.K, Kf, w, d, live);
            if (d < p.S && live) mr_store8<CL>(p.V0, c, b, d, p.S, h, p.H, w, p.W);
            if (d < p.M) {
                fold(a1, Ps0, d % K0, c);
                if (d % K0 == K0 - 1) {
                    if (live) mr_store8<CL>(p.V1, a1, b, d / K0, D1, h, p.H, w, p.W);
#pragma unroll
                    for (int o = 0; o < MR_G; ++o) a1[o] = 0.f;
                }
            }
            fold(a2, Ps1, d % K1, c);
            if (d % K1 == K1 - 1) {
                if (live) mr_store8<CL>(p.V2, a2, b, d / K1, D2, h, p.H, w, p.W);
#pragma unroll
                for (int o = 0; o < MR_G; ++o) a2[o] = 0.f;
            }
        }
        if constexpr (KT > 0) {
            if (more) mr_commit<CT, 256>(ring, nb, xn, tid);
            __syncthreads();
        }
    }
}

}  // namespace osa

extern "C" int osa_mr_volume_f32(const float* left, const float* right, const float* patch0, const float* patch1, float* v0, float* v1, float* v2, int layout,
                                 int B, int C, int H, int W, int num_groups, int out_channels, int maxdisp, int s_range, int m_range, int k0, int k1, void* stream) {
    if (int rc = mr_check("mr_volume", left && right && patch0 && patch1 && v0 && v1 && v2, B, C, H, W, num_groups, out_channels, maxdisp, s_range, m_range, k0, k1, layout)) return rc;
    MrArgs a{left, right, patch0, patch1, v0, v1, v2, nullptr, nullptr, nullptr, B, C, H, W, maxdisp, s_range, m_range, C / num_groups, cdiv(W, MR_WT), 0};
    a.DCH = mr_chunk(B * H * a.nWt, maxdisp);
    mr_dispatch(a.K, k0, k1, layout, [&](auto kt, auto c0, auto c1, auto cl) {
        hipLaunchKernelGGL((mr_volume_fwd_kernel<decltype(kt)::value, decltype(c0)::value, decltype(c1)::value, decltype(cl)::value>),
                           dim3(B * H * a.nWt, cdiv(maxdisp, a.DCH)), dim3(256), 0, (hipStream_t)stream, a);
    });
    OSA_LAUNCH_CHECK("mr_volume");
    return 0;
}
