// Output-plane-walking form of the fused stride-2 TRANSPOSED 3x3x3 convolutions (k = 3, p = 1, op = 1; f16x3 mode, split input, split
// output, split redir input): conv5 / conv6 of the GwcNet hourglasses with their 1x1x1 `redir` branch.
//
// The brick kernel (conv_mfma_kernel<.. NCLS = 8 ..>) carries all 8 output-parity classes of a 4 x 4 x 8 brick at once: 128 accumulator
// registers at MT = NT = 1, a 5 x 5 x 9 halo brick per 128 positions, Cout = 64 as two workgroups that stage the same input, and the
// redir input and the output touched one class after the other in a synchronous epilogue.  Here a workgroup owns TH x 32 INPUT pixels
// (2 TH x 64 output pixels per output plane) and walks a segment of OUTPUT planes:
//   * output plane 2a needs input plane a only (kd = 1: 9 (kh, kw) taps over the four (h, w) parity classes); plane 2a + 1 needs plane a
//     (kd = 2) and plane a + 1 (kd = 0): 18 taps.  Only the 4 (h, w) classes of ONE output plane are live: 4 accumulator sets x MT = 2
//     M-tiles per wave (128 accumulator registers, 2 waves per SIMD) -- every B fragment feeds two MFMA triples;
//   * Cout = 64 splits the waves over N inside the workgroup (2 x 2 waves): the input is staged once for both halves;
//   * a pass = (output plane, source plane, 16-channel chunk) = 3 steps (kh) of 3 taps (kw).  The chunk-plane of pass q + 1, with its +1
//     halo on the high h / w side, lands by LDS-DMA in the other plane buffer while pass q multiplies; the weights of step t + 2 land in
//     a 3-slot LDS ring, one fetch per workgroup and step.  Barrier / vmcnt protocol: conv_march_s2.h (tests/test_deconv_walk_taps_cpu.py
//     executes it).  An input chunk-plane is staged up to three times (by output planes 2a - 1, 2a, 2a + 1) -- the input is the small
//     tensor of these layers -- and a segment has no boundary planes;
//   * when an output plane is complete, every wave finalises its 8 tiles (class, M-tile): redir rows in A-operand order -> 3 MFMAs per
//     redir chunk -> z = fma(acc, s, t) + fma(R, s_r, t_r) in accumulator layout (the brick form's arithmetic, same order) -> activation
//     -> transpose through a wave-private LDS tile -> 16-byte split stores.  The redir rows of tile i + 1 are requested before tile i
//     is processed; the other workgroup of the CU multiplies meanwhile.
// The packed weight stream is the brick kernel's (class-major taps): ConvArgs::toff[kd * 9 + kh * 3 + kw] holds the stream index of
// a tap (host: derived from cls_end / td / th / tw).  Same split arithmetic and operand ranges as conv_mfma_kernel; the summation ORDER of
// the taps differs (source plane outermost), so results agree with the brick form to fp32 rounding, not bitwise.
#pragma once
#include "conv_march_s2.h"

namespace osa {

// WN = 1: Cout = 32, 4 x 1 waves, an 8 x 32 input-pixel tile; WN = 2: Cout = 64, 2 x 2 waves, a 4 x 32 tile.
template <int WN_>
struct DeconvWalkGeo {
    static constexpr int NWV = 4, WN = WN_, WM = NWV / WN_, MT = 2, TW = 32, TH = WM * MT;
    static constexpr int LH = TH + 1, LW = TW + 1, VQ = 5, ROWQ = LW * VQ;   // halo on the high side only; voxels 80 B apart (conflict-free ds_read_b128)
    static constexpr int NPI = (LH * ROWQ + 63) / 64;                        // LDS-DMA instructions per chunk-plane
    static constexpr int TILEQ = NWV * 32 * 36 / 4;                          // float4 slots of the epilogue's wave-private transpose tiles
    static constexpr int PLANEQ = (NPI * 64 > TILEQ) ? NPI * 64 : TILEQ;     // float4 slots per plane buffer (the tiles alias the buffer whose taps are done)
    static constexpr int NP = (NPI + NWV - 1) / NWV;                         // pieces per wave and pass
    static constexpr int BRING = 3, NFRAG = 6 * WN_, BSTEPQ = NFRAG * 64;    // ring slots; fragments f = (kw * 2 + hl) * WN + n of 1 KB per step
    static constexpr int NIB = (NFRAG + NWV - 1) / NWV;                      // B transfers per wave and step (WN = 1: 8 issued for 6 fragments, 2 duplicates)
    static constexpr size_t lds_bytes() { return (size_t)2 * PLANEQ * 16 + (size_t)BRING * BSTEPQ * 16; }
    static_assert(NIB + NP <= 9, "vmcnt immediates of the step waits");
};

// RCH: 16-channel chunks of the redir input (2: weights held in registers; 4: read in place)
template <int WN_, int RCH>
__global__ __launch_bounds__(256, 2) void conv_deconv_walk_kernel(const ConvArgs p, const int oseg, const int nseg) {
    using G = DeconvWalkGeo<WN_>;
    constexpr int PLANEQ = G::PLANEQ, NP = G::NP, NPI = G::NPI, NWV = G::NWV, NIB = G::NIB, WN = G::WN, MT = G::MT, TH = G::TH, TW = G::TW,
                  ROWQ = G::ROWQ, VQ = G::VQ;
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    float4* const bring = smem + 2 * PLANEQ;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wv / WN, wn = wv % WN;                      // M group (MT input rows), N-tile (32 output channels)
    const int col = lane & 31, hh = lane >> 5;

    unsigned bid = xcd_remap(blockIdx.x, gridDim.x);
    const int twi = bid % p.tilesW; bid /= p.tilesW;
    const int thi = bid % p.tilesH; bid /= p.tilesH;
    const int seg = bid % nseg;
    const int b = (int)(bid / nseg);
    const int o0 = seg * oseg, o1 = (o0 + oseg < p.Do) ? o0 + oseg : p.Do;
    const int a0h = thi * TH, a0w = twi * TW;

    // ---- f16x3 operand ranges (as conv_mfma_kernel with split input / redir input / output)
    float s_in = 1.f, s_rx = 1.f, s_out = 1.f;
    if (p.in_meta) s_in = p.in_meta[1];
    if (p.rx_meta) s_rx = p.rx_meta[1];
    if (p.coef && p.in_meta) {
        float bound = p.coef[0] * amax_read(p.in_meta) + p.coef[1];
        if (p.rcoef && p.rx_meta) bound += p.rcoef[0] * amax_read(p.rx_meta) + p.rcoef[1];
        s_out = pow2_scale(bound * 1.0625f);
    }
    if (p.out_meta && blockIdx.x == 0 && tid == 0) p.out_meta[1] = s_out;
    const float osc = (p.wscale_dev ? p.wscale_dev[1] : p.oscale) * (1.0f / s_in);
    const float rosc = p.roscale * (1.0f / s_rx);
    float am = 0.f;
    unsigned amax_seen = 0u;
    if (p.out_meta) amax_seen = amax_peek(p.out_meta);

    f32x16 acc[4][MT];                                         // [(oh parity) * 2 + (ow parity)][M-tile] of the output plane being walked
    auto zero_acc = [&]() {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[c][m][r] = 0.f;
    };
    zero_acc();

    const int CoP = p.CoP;                                     // == 32 * WN
    const int nch = p.nchunks;
    const int c8 = (lane & 3) * 8, vs2 = lane >> 2;            // epilogue: 8 channels of 2 voxels per lane
    const int actk = p.act & 15;
    const float act_ns = (actk == OSA_ACT_NONE) ? 1.f : ((actk == OSA_ACT_LEAKY) ? p.slope : 0.f);
    const bool act_relu = actk == OSA_ACT_RELU;
    const size_t ovox_b = (size_t)b * p.Do * p.Ho * p.Wo;
    float* const yb = p.y + ovox_b * p.yCs;
    const float* const rxb = p.rx + ovox_b * p.rxCs;

    // per-lane (channel wn * 32 + col) BN factors of both branches, redir weights (1x1x1: one tap per chunk)
    const int cl = wn * 32 + col;
    const float s6 = p.scale ? p.scale[cl] * osc : osc, t6 = p.shift ? p.shift[cl] : 0.f;
    const float sr = p.rscale ? p.rscale[cl] * rosc : rosc, tr = p.rshift ? p.rshift[cl] : 0.f;
    const float4* const rwp = p.rw + (size_t)hh * CoP + cl;
    const int rbstep = 2 * CoP, rtstep = JO * rbstep;
    constexpr bool HOIST_W = (RCH == 2);
    float4 rwb[HOIST_W ? RCH : 1][2];
    if constexpr (HOIST_W) {
#pragma unroll
        for (int ch = 0; ch < RCH; ++ch) { rwb[ch][0] = rwp[ch * rtstep]; rwb[ch][1] = rwp[ch * rtstep + rbstep]; }
    }

    // ---- LDS-DMA (conv_march.h: every instruction is issued by every wave with all lanes on; the vmcnt immediates count instructions)
    auto dma = [&](const char* src, const unsigned lds_byte) { lds_dma16(src, lds_byte); };
    const unsigned smem_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    const unsigned bring_lds = smem_lds + 2u * PLANEQ * 16u;
    const char* const zsrc = reinterpret_cast<const char*>(g_lds_dma_zeros);

    // B: a step's fragments f = (kw * 2 + hl) * WN + n, 64 lanes x 16 B each.  WN = 1: wave w fetches fragment w and fragment 4 + (w & 1)
    // (waves 2, 3 repeat 4, 5: the same bytes to the same slots); WN = 2: fragments 3 w .. 3 w + 2.
    // packed weights: 16-byte unit ((ch * 27 + t) * 4 + hl * 2 + kg) * CoP + co, t = stream index of the tap (class-major)
    int bkw[NIB];
    unsigned boff[NIB], bdst[NIB];
#pragma unroll
    for (int i = 0; i < NIB; ++i) {
        const int f = (WN == 1) ? (i == 0 ? wv : 4 + (wv & 1)) : wv * 3 + i;
        const int hl = (f / WN) & 1, n = f % WN;
        bkw[i] = f / (2 * WN);
        boff[i] = (unsigned)(((hl * 2 + hh) * CoP + n * 32 + col) * 16);
        bdst[i] = (unsigned)(f * 64 * 16);
    }
    auto dma_b = [&](const int slot, const int ch, const int kd, const int kh) {
        const char* base = reinterpret_cast<const char*>(p.w) + (size_t)(ch * 27) * (4 * CoP * 16);
#pragma unroll
        for (int i = 0; i < NIB; ++i) {
            const int t = p.toff[kd * 9 + kh * 3 + bkw[i]];
            dma(base + (size_t)t * (4 * CoP * 16) + boff[i], bring_lds + (unsigned)(slot * G::BSTEPQ * 16) + bdst[i]);
        }
    };

    // planes: piece i of this wave is DMA instruction n = i * NWV + wave (beyond NPI - 1: instruction NPI - 1 again).  LDS slot j = 64 n + lane
    // -> (row lh, voxel lw, quad c4) of the padded image; its source inside the (plane, chunk) slab, or the zero block for the padding slot
    // and for pixels outside the image (the high-side halo of the last tiles).
    unsigned poff[NP];
    unsigned pvalid = 0u;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        int n = i * NWV + wv;
        n = n < NPI ? n : NPI - 1;
        const int j = n * 64 + lane;
        const int lh = j / ROWQ, rem = j - lh * ROWQ, lw = rem / VQ, c4 = rem - lw * VQ;
        const int gh = a0h + lh, gw = a0w + lw;
        const bool ok = lh < G::LH && c4 < 4 && gh < p.Hi && gw < p.Wi;
        poff[i] = ok ? (unsigned)(((gh * p.Wi + gw) * p.xCs + c4 * 4) * 4) : 0u;
        pvalid |= ok ? (1u << i) : 0u;
    }
    const size_t plane_bytes = (size_t)p.Hi * p.Wi * p.xCs * 4;
    const char* const xb = reinterpret_cast<const char*>(p.x) + (size_t)b * p.Di * plane_bytes;
    auto dma_plane = [&](const int buf, const int pd, const int c) {          // pd < 0: nothing to fetch (zeros: the instruction count stays the same)
        const char* base = xb + (size_t)(pd < 0 ? 0 : pd) * plane_bytes + (size_t)c * (CC * 4);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            int n = i * NWV + wv;
            n = n < NPI ? n : NPI - 1;
            const bool ok = ((pvalid >> i) & 1u) && pd >= 0;
            dma(ok ? base + poff[i] : zsrc, smem_lds + (unsigned)((buf * PLANEQ + n * 64) * 16));
        }
    };

    // ---- one step: the 3 kw taps of kernel row KH from plane buffer `cur`, B fragments from ring slot `slot`: 9 MT MFMAs.
    // kh = 1 feeds the even output rows from input row r; kh = 0 the odd rows from r + 1, kh = 2 the odd rows from r (w alike).
    auto taps = [&](auto KH_, const int cur, const int slot) {
        constexpr int KH = decltype(KH_)::value;
        constexpr int ph = (KH != 1) ? 1 : 0, dh = (KH == 0) ? 1 : 0;
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int pw = (kw != 1) ? 1 : 0, dw = (kw == 0) ? 1 : 0;
            float4 A[MT][2], Bf[2];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int v = cur * PLANEQ + (wm * MT + m + dh) * ROWQ + (col + dw) * VQ + hh;
                A[m][0] = smem[v]; A[m][1] = smem[v + 2];
            }
            Bf[0] = bring[slot * G::BSTEPQ + ((kw * 2 + 0) * WN + wn) * 64 + lane];
            Bf[1] = bring[slot * G::BSTEPQ + ((kw * 2 + 1) * WN + wn) * 64 + lane];
#pragma unroll
            for (int term = 0; term < 3; ++term)                      // small cross terms first (as the other forms)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const f16x8 a = __builtin_bit_cast(f16x8, A[m][term == 1 ? 1 : 0]);
                    const f16x8 w = __builtin_bit_cast(f16x8, Bf[term == 0 ? 1 : 0]);
                    acc[ph * 2 + pw][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, w, acc[ph * 2 + pw][m], 0, 0, 0);
                }
        }
    };

    // ---- epilogue of the finished output plane od: redir branch on the MFMA, BN of both branches, activation, split NDHWC store
    auto epilogue = [&](const int od, float* const tb) {
        // redir rows of tile i = cls * MT + m in A-operand order: lane (col, hh) -> output voxel (od, 2 ih + ph, 2 (a0w + col) + pw); row k = 2 ch + j
        // of chunk ch: j = 0 the lane's 8 hi halves, j = 1 its 8 lo halves
        constexpr int RV = 2 * RCH;
        auto load_x = [&](const int i, float4 (&rv)[RV]) {
            const int c = i / MT, m = i % MT;
            const int ih = a0h + wm * MT + m, iw = a0w + col;
            const bool ok = ih < p.Hi && iw < p.Wi;
            const int vox = (od * p.Ho + 2 * ih + (c >> 1)) * p.Wo + 2 * iw + (c & 1);
#pragma unroll
            for (int k = 0; k < RV; ++k) {
                rv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok) rv[k] = *reinterpret_cast<const float4*>(rxb + vox * p.rxCs + (k >> 1) * CC + 4 * hh + 8 * (k & 1));
            }
        };
        // ONE register set of rows: the rows of tile i + 1 are requested as soon as the MFMAs of tile i have read theirs, so their round trip
        // overlaps the transpose, arithmetic and stores of tile i
        float4 rv[RV];
        load_x(0, rv);
#pragma unroll
        for (int i = 0; i < 4 * MT; ++i) {
            const int c = i / MT, m = i % MT;
            f32x16 r;
#pragma unroll
            for (int e = 0; e < 16; ++e) r[e] = 0.f;
#pragma unroll
            for (int ch = 0; ch < RCH; ++ch) {
                float4 b0, b1;
                if constexpr (HOIST_W) { b0 = rwb[ch][0]; b1 = rwb[ch][1]; }
                else { b0 = rwp[ch * rtstep]; b1 = rwp[ch * rtstep + rbstep]; }
                const f16x8 ah = __builtin_bit_cast(f16x8, rv[2 * ch]), al = __builtin_bit_cast(f16x8, rv[2 * ch + 1]);
                const f16x8 bh = __builtin_bit_cast(f16x8, b0), bl = __builtin_bit_cast(f16x8, b1);
                r = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, r, 0, 0, 0);
                r = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, r, 0, 0, 0);
                r = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, r, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (i + 1 < 4 * MT) load_x(i + 1, rv);
            // registers -> LDS (tile[voxel][channel], row stride 36 floats), both branches' BN applied in accumulator layout
#pragma unroll
            for (int e = 0; e < 16; ++e) tb[((e & 3) + 8 * (e >> 2) + 4 * hh) * 36 + col] = fmaf(acc[c][m][e], s6, t6) + fmaf(r[e], sr, tr);
            const int ih = a0h + wm * MT + m;
            const int soff = wn * 32 + (c8 >> 4) * 16 + ((c8 & 15) >> 3) * 4;      // float offset of this lane's 8 hi halves inside the voxel
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int iw = a0w + vs2 + 16 * k;
                const bool ok = ih < p.Hi && iw < p.Wi;
                const int vox = (od * p.Ho + 2 * ih + (c >> 1)) * p.Wo + 2 * iw + (c & 1);
                uint2 hq[2], lq[2];
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const float4 a = *reinterpret_cast<const float4*>(tb + (vs2 + 16 * k) * 36 + c8 + 4 * h2);
                    float o[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (o[e] < 0.f) ? (act_relu ? 0.f : o[e] * act_ns) : o[e];
                    if (ok) am = fmaxf(am, fmaxf(fmaxf(fabsf(o[0]), fabsf(o[1])), fmaxf(fabsf(o[2]), fabsf(o[3]))));
                    split_f16(make_float4(o[0] * s_out, o[1] * s_out, o[2] * s_out, o[3] * s_out), hq[h2], lq[h2]);
                }
                if (ok) {
                    float* ys = yb + vox * p.yCs + soff;
                    store16(ys, make_uint4(hq[0].x, hq[0].y, hq[1].x, hq[1].y));
                    store16(ys + 8, make_uint4(lq[0].x, lq[0].y, lq[1].x, lq[1].y));
                }
            }
            __builtin_amdgcn_sched_barrier(0);                // tiles are scheduled one at a time: bounds live ranges
        }
    };

    // ---- pass / step sequence.  Output plane od = 2a + par has nsrc source planes: par = 0: plane a (kd = 1); par = 1: plane a (kd = 2)
    // and, if it exists, plane a + 1 (kd = 0).  Pass = (od, source j, chunk c), 3 steps (kh); global step t uses ring slot t % 3.
    auto nsrc = [&](const int od) { return (od & 1) ? (((od >> 1) + 1 < p.Di) ? 2 : 1) : 1; };
    auto kd_of = [&](const int od, const int j) { return (od & 1) ? (j == 0 ? 2 : 0) : 1; };
    // look-ahead iterator of the B transfers (two steps ahead of the step being computed); past the end it stays on the last step
    int lod = o0, lj = 0, lc = 0, lk = 0;
    bool ldone = false;
    auto issue_b = [&](const int slot) {
        dma_b(slot, lc, kd_of(lod, lj), lk);
        if (!ldone) {
            if (++lk == 3) {
                lk = 0;
                if (++lc == nch) { lc = 0; if (++lj == nsrc(lod)) { lj = 0; ++lod; } }
                if (lod >= o1) { ldone = true; lod = o1 - 1; lj = nsrc(lod) - 1; lc = nch - 1; lk = 2; }
            }
        }
    };

    dma_plane(0, o0 >> 1, 0);
    issue_b(0); issue_b(1);
    wait_vmcnt_c<0>();

    int slot = 0;                                             // ring slot of the step being computed
    int q = 0;
    for (int od = o0; od < o1; ++od) {
        const int ns = nsrc(od);
        int cur = 0;
        for (int j = 0; j < ns; ++j)
            for (int c = 0; c < nch; ++c, ++q) {
                cur = q & 1;
                // plane-chunk of pass q + 1
                int nod = od, nj = j, nc = c + 1;
                if (nc == nch) { nc = 0; if (++nj == ns) { nj = 0; ++nod; } }
                const int npd = (nod < o1) ? (nod >> 1) + nj : -1;
                // every step: barrier (every wave's share of this step's B -- and, at kh = 0, of this pass's plane -- has landed; the previous
                // step's readers of ring slot (slot + 2) % 3 are done), B of step t + 2 -> slot (t + 2) % 3, taps, then the wait that brings
                // B of step t + 1 home (younger: this step's B transfer and -- during steps 0 and 1 -- the plane pieces)
                __syncthreads();
                issue_b(slot >= 1 ? slot - 1 : 2);
                dma_plane(cur ^ 1, npd, nc);
                taps(std::integral_constant<int, 0>{}, cur, slot);
                wait_vmcnt_c<NIB + NP>();
                slot = slot == 2 ? 0 : slot + 1;

                __syncthreads();
                issue_b(slot >= 1 ? slot - 1 : 2);
                taps(std::integral_constant<int, 1>{}, cur, slot);
                wait_vmcnt_c<NIB + NP>();
                slot = slot == 2 ? 0 : slot + 1;

                __syncthreads();
                issue_b(slot >= 1 ? slot - 1 : 2);
                taps(std::integral_constant<int, 2>{}, cur, slot);
                wait_vmcnt_c<NIB>();
                slot = slot == 2 ? 0 : slot + 1;
            }
        __syncthreads();                                      // every wave is past its taps: buffer `cur` becomes the transpose tiles
        epilogue(od, reinterpret_cast<float*>(smem + cur * PLANEQ) + wv * (32 * 36));
        zero_acc();
    }
    wait_vmcnt_c<0>();                                            // (the zero pieces / spare B transfers of the last pass)
    if (p.out_meta) {
        __syncthreads();
        publish_amax(p.out_meta, am, amax_seen, reinterpret_cast<float*>(smem));
    }
}

}  // namespace osa
