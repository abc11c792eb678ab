// Geometry-encoding volume of StereoBase / IGEV's GRU loop.
//   reference: models/stereobase/gru_blocks.py:170-229 (CombinedGeoEncodingVolume),
//              models/igev/geometry.py:7-66 (Combined_Geo_Encoding_Volume)
//  * allpairs_corr : corr[b,h,w1,w2] = sum_c f1[b,c,h,w1] * f2[b,c,h,w2]          (einsum 'aijk,aijh->ajkh')
//  * geo_rows      : NDHWC geometry volume -> per-pixel rows [B,H,W,C,D] (the reference's
//                    permute(0,3,4,1,2).reshape(b*h*w, c, 1, d)), lookup-friendly: one row = D contiguous floats
//  * avgpool_rows  : F.avg_pool2d(x, [1,2], stride=[1,2]) along the last axis -> pyramid level i+1
//  * geo_lookup    : for every pixel, level and channel row: 2r+1 taps at x = pos/2^i + (k - r), 1-D linear
//                    interpolation with zero padding (grid_sample, align_corners=True, H == 1), for the C geometry
//                    rows (pos = disp) and the correlation row (pos = coords - disp); writes the reference's
//                    [B, (C+1)*(2r+1)*levels, H, W] tensor in one pass instead of 4 grid_sample calls + cats per iteration.
// All memory-bound; lanes run along w (outputs) or along the contiguous row axis (transposes).
#include "osa_common.h"
#include <cstring>
#include <type_traits>

namespace osa {

// ---- all-pairs correlation: block = (b, h, 16 left pixels); thread = right pixel
__global__ __launch_bounds__(256) void allpairs_corr_kernel(const float* __restrict__ f1, const float* __restrict__ f2,
                                                            float* __restrict__ corr, int C, int H, int W1, int W2) {
    extern __shared__ float f1s[];                 // [C][16]
    const int tiles = (W1 + 15) / 16;
    int bid = blockIdx.x;
    const int t = bid % tiles; bid /= tiles;
    const int h = bid % H; const int b = bid / H;
    const int w10 = t * 16;
    const size_t plane1 = (size_t)H * W1, plane2 = (size_t)H * W2;
    for (int i = threadIdx.x; i < C * 16; i += 256) {
        const int c = i >> 4, j = i & 15;
        f1s[i] = (w10 + j < W1) ? f1[((size_t)b * C + c) * plane1 + (size_t)h * W1 + w10 + j] : 0.f;
    }
    __syncthreads();
    for (int w2 = threadIdx.x; w2 < W2; w2 += 256) {
        float acc[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.f;
        const float* r = f2 + (size_t)b * C * plane2 + (size_t)h * W2 + w2;
        for (int c = 0; c < C; ++c) {
            const float v = r[(size_t)c * plane2];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc[j] = fmaf(f1s[c * 16 + j], v, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (w10 + j < W1) corr[(((size_t)b * H + h) * W1 + w10 + j) * W2 + w2] = acc[j];
    }
}

// ---- NDHWC volume [B,D,H,W,Cs] -> rows [B,H,W,C,D]; block = (b, h, 8 pixels)
__global__ __launch_bounds__(256) void geo_rows_kernel(const float* __restrict__ vol, float* __restrict__ rows,
                                                       int D, int H, int W, int C, int Cs) {
    extern __shared__ float tile[];                // [8][D][C+1]
    const int tiles = (W + 7) / 8;
    int bid = blockIdx.x;
    const int t = bid % tiles; bid /= tiles;
    const int h = bid % H; const int b = bid / H;
    const int w0 = t * 8, CP = C + 1;
    const int n_in = 8 * D * C;
    for (int i = threadIdx.x; i < n_in; i += 256) {       // c fastest: coalesced C-vectors
        const int c = i % C; int r = i / C;
        const int px = r % 8; const int d = r / 8;
        float v = 0.f;
        if (w0 + px < W) v = vol[((((size_t)b * D + d) * H + h) * W + w0 + px) * Cs + c];
        tile[(px * D + d) * CP + c] = v;
    }
    __syncthreads();
    const int n_out = 8 * C * D;
    for (int i = threadIdx.x; i < n_out; i += 256) {      // d fastest: one pixel's [C][D] block is contiguous
        const int d = i % D; int r = i / D;
        const int c = r % C; const int px = r / C;
        if (w0 + px < W) rows[((((size_t)b * H + h) * W + w0 + px) * C + c) * D + d] = tile[(px * D + d) * CP + c];
    }
}

__global__ __launch_bounds__(256) void avgpool_rows_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                           long long rows, int n) {
    const int no = n / 2;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * no) return;
    const long long r = i / no; const int j = (int)(i - r * no);
    const float* p = x + r * n + 2 * j;
    y[i] = (p[0] + p[1]) * 0.5f;
}

// Sampling position of one tap, with the reference's own float roundings: bilinear_sampler (igev/utils.py:61-79) maps the
// pixel coordinate x to xgrid = 2 * x / (n - 1) - 1 and F.grid_sample(align_corners=True) maps it back with
// ((xgrid + 1) / 2) * (n - 1); at n = 240 the round trip moves x by up to ~2e-5, which shifts the interpolation weights.
// Reproducing the round trip keeps the lookup within a few 1e-6 of the reference at any width (-ffp-contract=off: no fma).
struct Tap { int x0; float w0, w1; };
__device__ __forceinline__ Tap tap_of(float x, int n) {
    const float nm1 = (float)(n - 1);
    const float g = 2.f * x / nm1 - 1.f;
    const float ix = ((g + 1.f) / 2.f) * nm1;
    const float xf = floorf(ix);
    Tap t;
    t.x0 = (int)xf;
    t.w1 = ix - xf;
    t.w0 = (xf + 1.f) - ix;
    return t;
}
__device__ __forceinline__ float sample_row(const float* __restrict__ row, int n, const Tap t) {
    const float a = (t.x0 >= 0 && t.x0 < n) ? row[t.x0] : 0.f;
    const float b = (t.x0 + 1 >= 0 && t.x0 + 1 < n) ? row[t.x0 + 1] : 0.f;
    return a * t.w0 + b * t.w1;
}

// ---- the lookup kernels.  Two lookups run on them: the single pyramid of StereoBase / IGEV (models/igev/geometry.py) and the multi-range
// lookup of IGEV++ (models/igevpp/geometry.py:6-87): volume 0 with an averaged pyramid at disp / 2^l, volumes 1 and 2 (no pyramid) at
// disp / 2 and disp / 4, the correlation pyramid at coords / 2^l - disp / 2^l; four output tensors (geo_feat0 / 1 / 2, init_corr).
// The channels-last body is written once; the NCHW forward and the accumulating backward are written out for each lookup (see there).
// A body works on the description of one row of a pixel, LookupSrc: the rows, their length, rows per pixel, an exact power-of-two scale,
// the kind of position, where the taps go.  The lookups differ only in how row j finds that description.  That is the shared kernel's template
// parameter P: MultiLookupArgs, a short list of sources passed by value (IGEV++), or LevelTable, where j = l * (C + 1) + c is row c of
// level l (c == C: the correlation row) and the description is arithmetic over a table of levels.
struct LookupSrc {
    const float* rd;         // forward: the rows [B,H,W,rows,n]; backward: the upstream gradient of the tensor the rows' taps went to
    float* wr;               // forward: the tensor the taps go to; backward: the gradient accumulator of the rows
    int n, rows;             // row length; rows per pixel (C, or 1 for a correlation level)
    int row0;                // list: index of the source's first row in a pixel's row list (ascending over the sources)
    int ch0, nch;            // first channel of the source in its tensor; the tensor's channel count (NCHW) / channel stride (channels-last)
    int pad_from;            // channels-last: the source that ends its tensor zero-fills channels pad_from .. nch - 1 (others: pad_from = nch)
    float scale;             // 1, 1/2, 1/4, 1/8
    int corr;                // 0: x = d * scale (geometry rows), 1: x = cx * scale - d * scale (correlation rows)
};
struct LookupRow { LookupSrc s; int c; };                                // a row's source and its index among the source's rows
__device__ __forceinline__ float src_pos(const LookupSrc& s, float d, float cx) {
    return s.corr ? cx * s.scale - d * s.scale : d * s.scale;
}

constexpr int MR_MAX_SRC = 10;                                           // 2 * levels + 2, levels <= 4
struct MultiLookupArgs {
    LookupSrc src[MR_MAX_SRC];
    const float* disp; const float* coords;
    int nsrc, rows_per_px, B, H, W, radius;
};
// the source of row j of a pixel.  The loop index is uniform, so the descriptors stay scalar loads from the kernel arguments and a lane picks
// its own by selects (indexing src[] by a per-lane value would put the whole list into scratch memory)
__device__ __forceinline__ LookupSrc src_of_row(const MultiLookupArgs& p, int j) {
    LookupSrc s = p.src[0];
#pragma unroll
    for (int q = 1; q < MR_MAX_SRC; ++q)
        if (q < p.nsrc && j >= p.src[q].row0) s = p.src[q];
    return s;
}
__device__ __forceinline__ LookupRow row_of(const MultiLookupArgs& p, int j, int /*TAPS*/) {
    LookupRow r;
    r.s = src_of_row(p, j);
    r.c = j - r.s.row0;
    return r;
}

// RowT / TensorT: const float / float forward (rows read, `t` written), float / const float backward (gradient rows accumulated into, `t` the
// upstream gradient read)
template <class RowT, class TensorT>
struct LevelTable {
    RowT* geo[4]; RowT* corr[4];                    // per level: rows [B,H,W,C,Dl] / [B,H,W,Wl]
    const float* disp; const float* coords; TensorT* t;
    int B, H, W, C, levels, radius;
    int Dl[4], Wl[4];
    int rows_per_px, nch;                           // levels * (C + 1); channel count of `t` (NCHW) / its channel stride (channels-last)
};
template <class RowT, class TensorT>
__device__ __forceinline__ LookupRow level_row(const LevelTable<RowT, TensorT>& p, int l, int c, int TAPS) {     // TAPS: the kernel's (0 = generic)
    const int taps = TAPS ? TAPS : 2 * p.radius + 1;
    const bool corr = c == p.C;
    const int per_level = (p.C + 1) * taps;
    RowT* rows = corr ? p.corr[l] : p.geo[l];
    LookupRow r;
    if constexpr (std::is_const_v<RowT>) { r.s.rd = rows; r.s.wr = p.t; } else { r.s.rd = p.t; r.s.wr = rows; }
    r.s.n = corr ? p.Wl[l] : p.Dl[l];
    r.s.rows = corr ? 1 : p.C;
    r.s.row0 = 0;
    r.s.ch0 = l * per_level + (corr ? p.C * taps : 0);
    r.s.nch = p.nch;
    r.s.pad_from = corr && l == p.levels - 1 ? p.levels * per_level : p.nch;
    r.s.scale = __int_as_float((127 - l) << 23);    // 2^-l from its exponent field, no division (the dense backward kernels multiply 0.5f l times)
    r.s.corr = corr;
    r.c = corr ? 0 : c;
    return r;
}
template <class RowT, class TensorT>
__device__ __forceinline__ LookupRow row_of(const LevelTable<RowT, TensorT>& p, int j, int TAPS) {
    const int l = j / (p.C + 1);
    return level_row(p, l, j - l * (p.C + 1), TAPS);
}

// NCHW (the training path), one thread per (row, pixel) (r5): a thread produces the 2r + 1 taps of ONE row (geometry row c of a source, or a
// correlation row) of one pixel; consecutive threads are consecutive pixels of the same row, so every store instruction of a wave
// writes consecutive floats of one output plane.  (One thread per PIXEL gave B*H*W threads -- 14720 at the StereoBase training map, 80 x 184,
// under one wave per SIMD of the chip -- each walking 324 scattered loads: profiles/DESIGN_rounds1-5.md.)
__global__ __launch_bounds__(256) void geo_lookup_rows_kernel(const MultiLookupArgs p) {
    const long long HW = (long long)p.H * p.W, npix = (long long)p.B * HW;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix * p.rows_per_px) return;
    const int j = (int)(t / npix);                                  // row (uniform over a workgroup unless it straddles a row boundary)
    const long long i = t - (long long)j * npix;                    // pixel
    const long long b = i / HW, hw = i - b * HW;
    const LookupSrc s = src_of_row(p, j);
    const int c = j - s.row0;
    const int taps = 2 * p.radius + 1;
    const float x = src_pos(s, p.disp[i], p.coords[i]);
    const float* row = s.rd + ((size_t)i * s.rows + c) * s.n;
    float* o = s.wr + ((size_t)b * s.nch + s.ch0 + (size_t)c * taps) * HW + hw;
    for (int k = 0; k < taps; ++k) {
        const float dx = (float)(k - p.radius);
        o[(size_t)k * HW] = sample_row(row, s.n, tap_of(s.corr ? x + dx : dx + x, s.n));       // operand order of geometry.py:36 / :44, igevpp/geometry.py:43,49,57 / :65
    }
}

// The same over the level table.  Written out beside the list form: as one body over a row finder (like the channels-last kernel) it
// gave the same values and was 0.2 - 0.7 % slower at 4 x 136 x 240 in every run (profiles/round11/lookup_one_definition.md).
__global__ __launch_bounds__(256) void geo_lookup_level_rows_kernel(const LevelTable<const float, float> p) {
    const long long HW = (long long)p.H * p.W, npix = (long long)p.B * HW;
    const int rows_per_px = p.levels * (p.C + 1);
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= npix * rows_per_px) return;
    const int j = (int)(t / npix);                                  // row
    const long long i = t - (long long)j * npix;                    // pixel
    const long long b = i / HW, hw = i - b * HW;
    const int l = j / (p.C + 1), c = j - l * (p.C + 1);
    const int taps = 2 * p.radius + 1;
    const int per_level = (p.C + 1) * taps;
    float scale = 1.f;
    for (int q = 0; q < l; ++q) scale *= 0.5f;
    const float d = p.disp[i], cx = p.coords[i];
    const bool is_corr = (c == p.C);
    const int n = is_corr ? p.Wl[l] : p.Dl[l];
    const float* row = is_corr ? p.corr[l] + (size_t)i * p.Wl[l] : p.geo[l] + ((size_t)i * p.C + c) * p.Dl[l];
    const float xg = d * scale, xc = cx * scale - d * scale;
    float* o = p.t + (size_t)b * per_level * p.levels * HW + hw + ((size_t)l * per_level + (size_t)c * taps) * HW;
    for (int k = 0; k < taps; ++k) {
        const float dx = (float)(k - p.radius);
        o[(size_t)k * HW] = sample_row(row, n, is_corr ? tap_of(xc + dx, n) : tap_of(dx + xg, n));      // operand order of geometry.py:36 / :44
    }
}

// The 2r + 1 taps of one row into 2r + 1 consecutive floats (the channels-last kernels): `x` is the row's position without the tap offset.
template <int TAPS>      // TAPS = 2 * radius + 1 known at compile time (9 in every shipped config), 0 = generic
__device__ __forceinline__ void row_taps_cl(const float* __restrict__ row, int n, float x, bool is_corr, int radius, float* __restrict__ o) {
    if constexpr (TAPS > 0) {
        // all loads first, unconditionally (index clamped into the row, the value dropped by a select): 2 * TAPS independent requests
        // in flight per thread instead of a branch and a wait per tap
        Tap tp[TAPS]; float a[TAPS], b[TAPS];
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float dx = (float)(k - TAPS / 2);
            tp[k] = tap_of(is_corr ? x + dx : dx + x, n);           // operand order of geometry.py:36 / :44
            const int i0 = tp[k].x0 < 0 ? 0 : (tp[k].x0 > n - 1 ? n - 1 : tp[k].x0);
            const int i1 = tp[k].x0 + 1 < 0 ? 0 : (tp[k].x0 + 1 > n - 1 ? n - 1 : tp[k].x0 + 1);
            a[k] = row[i0]; b[k] = row[i1];
        }
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float av = (tp[k].x0 >= 0 && tp[k].x0 < n) ? a[k] : 0.f;
            const float bv = (tp[k].x0 + 1 >= 0 && tp[k].x0 + 1 < n) ? b[k] : 0.f;
            o[k] = av * tp[k].w0 + bv * tp[k].w1;                   // == sample_row
        }
    } else {
        for (int k = 0; k < 2 * radius + 1; ++k) {
            const float dx = (float)(k - radius);
            o[k] = sample_row(row, n, tap_of(is_corr ? x + dx : dx + x, n));
        }
    }
}

// Channels-last form for the engine's GRU loop: out [B,H,W,Cs] (Cs >= channels, the padding zero-filled), i.e. what the update
// block's 1x1 convc1 reads -- the NCHW result of the kernel above had to be transposed every iteration (85 MB at 4 pairs).  One thread =
// one (pixel, row): it produces the 2r + 1 taps of its row = 2r + 1 consecutive channels of the row's tensor, so the threads of a pixel write
// its channel vector contiguously.  Same tap arithmetic (tap_of / sample_row), same values.
template <int TAPS, class P>
__global__ __launch_bounds__(256) void geo_lookup_nhwc_kernel(const P p) {
    const unsigned npix = (unsigned)p.B * p.H * p.W;                // host: B*H*W*rows < 2^31
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= npix * (unsigned)p.rows_per_px) return;
    const unsigned i = t / (unsigned)p.rows_per_px;
    const int j = (int)(t - i * (unsigned)p.rows_per_px);
    const LookupRow r = row_of(p, j, TAPS);
    const LookupSrc& s = r.s;
    const int taps = TAPS ? TAPS : 2 * p.radius + 1;
    const float x = src_pos(s, p.disp[i], p.coords[i]);
    float* px = s.wr + (size_t)i * s.nch;
    row_taps_cl<TAPS>(s.rd + ((size_t)i * s.rows + r.c) * s.n, s.n, x, s.corr != 0, p.radius, px + s.ch0 + r.c * taps);
    if (r.c == s.rows - 1)
        for (int k = s.pad_from; k < s.nch; ++k) px[k] = 0.f;
}

// Dense backward of the lookup w.r.t. the pyramid levels (the disparity is detached in the reference, igev_stereo.py:190), in GATHER form
// (r5): a thread owns one OUTPUT element (pixel, level, row, position j) and sums the taps that land on it: tap k contributes dout_k * w0_k
// if x0_k == j and dout_k * w1_k if x0_k + 1 == j, with the forward's tap_of(), in ascending order k = 0 .. 2r.  Every element is written
// (zeros included): no memset, no read-modify-write, consecutive threads write consecutive floats.  (The first form gave every pixel one
// thread that scattered its 324 terms into memset rows: 0.54 ms per call at the 80 x 184 training map, profiles/DESIGN_rounds1-5.md.)
struct LookupBwdGatherArgs {
    float* dgeo[4]; float* dcorr[4];
    const float* disp; const float* coords; const float* dout;
    int B, H, W, C, levels, radius;
    int Dl[4], Wl[4];
    long long seg_end[8];            // running end of segment 2 l (geo rows of level l) / 2 l + 1 (corr rows) in the flat element index
};
__global__ __launch_bounds__(256) void geo_lookup_bwd_gather_kernel(const LookupBwdGatherArgs p) {
    const long long HW = (long long)p.H * p.W;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int nseg = 2 * p.levels;
    if (t >= p.seg_end[nseg - 1]) return;
    int sgm = 0;
    while (t >= p.seg_end[sgm]) ++sgm;
    const long long e = t - (sgm ? p.seg_end[sgm - 1] : 0);
    const int l = sgm >> 1;
    const bool is_corr = sgm & 1;
    const int n = is_corr ? p.Wl[l] : p.Dl[l];
    const int rows = is_corr ? 1 : p.C;
    const int j = (int)(e % n);
    const long long r = e / n;
    const int c = is_corr ? p.C : (int)(r % rows);
    const long long i = is_corr ? r : r / rows;                        // pixel
    const long long b = i / HW, hw = i - b * HW;
    const int taps = 2 * p.radius + 1;
    const int per_level = (p.C + 1) * taps;
    float scale = 1.f;
    for (int q = 0; q < l; ++q) scale *= 0.5f;
    const float d = p.disp[i], cx = p.coords[i];
    const float xg = d * scale, xc = cx * scale - d * scale;
    const float* o = p.dout + (size_t)b * per_level * p.levels * HW + hw + ((size_t)l * per_level + (size_t)c * taps) * HW;
    float v = 0.f;
    for (int k = 0; k < taps; ++k) {
        const float dx = (float)(k - p.radius);
        const Tap tp = is_corr ? tap_of(xc + dx, n) : tap_of(dx + xg, n);
        if (tp.x0 == j) v += o[(size_t)k * HW] * tp.w0;
        if (tp.x0 + 1 == j) v += o[(size_t)k * HW] * tp.w1;
    }
    float* dst = is_corr ? p.dcorr[l] : p.dgeo[l];
    dst[e] = v;
}

// Gather form, one WAVE per (pixel, level) (r5, second version): the 2r + 1 tap positions of the level's geometry rows and of its correlation row
// are evaluated once per wave (they depend on the pixel only), a lane owns output positions j = lane, lane + 64, ... of every row, the
// upstream gradients of a row's taps are wave-uniform loads, and the lanes of a wave store consecutive floats.  The thread-per-element form
// above evaluates the same 9 taps for each of the C * D + W elements of the pixel.  Same taps, same order of additions: bit-identical.
template <int MAXT>
__global__ __launch_bounds__(256) void geo_lookup_bwd_rows_kernel(const LookupBwdGatherArgs p) {
    const long long HW = (long long)p.H * p.W;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long i = (long long)blockIdx.x * 4 + wv;                // pixel (wave-uniform)
    const int l = blockIdx.y;
    if (i >= (long long)p.B * HW) return;
    const int lane = threadIdx.x & 63;
    const long long b = i / HW, hw = i - b * HW;
    const int taps = 2 * p.radius + 1;                                  // <= MAXT (host)
    const int per_level = (p.C + 1) * taps;
    float scale = 1.f;
    for (int q = 0; q < l; ++q) scale *= 0.5f;
    const float d = p.disp[i], cx = p.coords[i];
    const float xg = d * scale, xc = cx * scale - d * scale;
    const int Dl = p.Dl[l], Wl = p.Wl[l];
    int gx0[MAXT], cx0[MAXT]; float gw0[MAXT], gw1[MAXT], cw0[MAXT], cw1[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) {
        const float dx = (float)(k - p.radius);
        const Tap tg = tap_of(dx + xg, Dl), tc = tap_of(xc + dx, Wl);
        const bool on = k < taps;
        gx0[k] = on ? tg.x0 : -4; gw0[k] = tg.w0; gw1[k] = tg.w1;       // (-4: matches no position j >= 0, nor j - 1)
        cx0[k] = on ? tc.x0 : -4; cw0[k] = tc.w0; cw1[k] = tc.w1;
    }
    // every upstream gradient of this (pixel, level) -- (C + 1) rows x taps, 81 in the shipped configs, each in its own output plane -- with ONE
    // round of loads (each lane holds up to four of them; host: (C + 1) * taps <= 256); the rows then take theirs by readlane.  (The first
    // version loaded a row's taps as wave-uniform values inside the row loop: C + 1 dependent memory round trips per wave, 237 us inside the
    // training step although the kernel moves 60 MB.)
    const float* o = p.dout + (size_t)b * per_level * p.levels * HW + hw + (size_t)l * per_level * HW;
    float gq[4];                                                         // lane t holds elements t, t + 64, t + 128, t + 192 (host: per_level <= 256)
#pragma unroll
    for (int v = 0; v < 4; ++v) gq[v] = lane + 64 * v < per_level ? o[(size_t)(lane + 64 * v) * HW] : 0.f;
    auto take = [&](int idx) -> float {                                  // idx wave-uniform
        const int s_ = __builtin_amdgcn_readfirstlane(idx);
        const int q = s_ >> 6;
        const float src = q == 0 ? gq[0] : (q == 1 ? gq[1] : (q == 2 ? gq[2] : gq[3]));
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(src), s_ & 63));
    };
    float* g = p.dgeo[l] + (size_t)i * p.C * Dl;
    for (int c = 0; c < p.C; ++c) {
        float ov[MAXT];
#pragma unroll
        for (int k = 0; k < MAXT; ++k) ov[k] = k < taps ? take(c * taps + k) : 0.f;
        for (int j = lane; j < Dl; j += 64) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < MAXT; ++k) {
                if (gx0[k] == j) v += ov[k] * gw0[k];
                if (gx0[k] + 1 == j) v += ov[k] * gw1[k];
            }
            g[(size_t)c * Dl + j] = v;
        }
    }
    float ov[MAXT];
#pragma unroll
    for (int k = 0; k < MAXT; ++k) ov[k] = k < taps ? take(p.C * taps + k) : 0.f;
    float* crow = p.dcorr[l] + (size_t)i * Wl;
    for (int j = lane; j < Wl; j += 64) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < MAXT; ++k) {
            if (cx0[k] == j) v += ov[k] * cw0[k];
            if (cx0[k] + 1 == j) v += ov[k] * cw1[k];
        }
        crow[j] = v;
    }
}


// Accumulating form (r6): the reference's loop looks the SAME pyramid up once per GRU iteration (igev_stereo.py:181-203: 22 iterations in
// training), so autograd used to receive 22 dense gradients per level (50 MB each at the 320x736 crop, 98 % zeros) and add them up.  Here
// the level gradients are accumulators the caller zero-fills once per step; a lookup's backward touches only the window of 2r + 3 positions
// per row of a (pixel, level) that its taps can reach: one lane per position, a read-modify-write without atomics (every pixel owns its
// rows, a lane owns its position) -- 2.6 M entries touched instead of 12.5 M written and 12.5 M added per iteration.
//
// Which position a tap reaches is tap_of()'s business alone.  Its float round trip returns an integer position k as k - eps or k + eps,
// and dx + x rounds differently from tap to tap, so consecutive taps do NOT always have consecutive x0: the step is 0 ("both taps reach
// the same two positions") or 2 ("the position between them belongs to the first tap alone") at a few per cent of the lattice positions.
// (The first version of this kernel took entry jj to be position x0(tap jj) = x0(tap jj - 1) + 1: it dropped the w1 term of the tap before
// a step of 2 and let two lanes add to one address at a step of 0.)  So the window is anchored once per row: lane e of a row owns position
// x0(tap 0) + e, e = 0 .. 2r + 2, and adds up, in ascending tap order (the order of the dense kernels: into zeros the result is theirs bit
// for bit), the w0 terms of the taps whose x0 is its position and the w1 terms of those whose x0 + 1 is.
// Why that window holds every term: tap k samples fl(dx_k + x) and tap_of() moves it by at most u * (4 |x| + n) (u = 2^-24; one rounding
// each in 2x / (n - 1), - 1, + 1, * (n - 1)), together under 0.4 for |x|, n <= 2^20 (host: n <= 2^19; farther out every tap is off the row
// and nothing is stored).  With every ix_k within 0.5 of x + dx_k and ix non-decreasing in k, x0(tap k) - x0(tap 0) is k - 1, k or k + 1:
// positions x0(tap 0) .. x0(tap 0) + 2r + 2, and position x0(tap 0) + e can only be reached by taps e - 2 .. e + 1.
// Lanes: a row takes G = 2r + 3 consecutive lanes of a wave, 64 / G rows per wave (5 of the 9-tap rows: 55 lanes).  Lane e < 2r + 1 evaluates
// tap e and loads its upstream gradient -- once per tap -- and the lanes of a row exchange (x0, g * w0, g * w1) by shuffles.

// The window of one row, shared by the accumulating kernels: lane e of the row's G = taps + 2 lanes (e < taps: tap e, whose upstream gradient is
// o[e * ostride]) adds what the taps e - 2 .. e + 1 put on position j = x0(tap 0) + e of its row, at entry(j) (asked for by the lanes that store only).
// Every lane of the wave calls it (shuffles).
template <class Entry>
__device__ __forceinline__ void acc_row_window(int taps, int lane, int e, bool row_on, float x, int n, const float* __restrict__ o, size_t ostride,
                                               Entry entry) {
    const Tap tk = tap_of((float)(e - taps / 2) + x, n);                 // (lanes e >= taps: evaluated, never used)
    const float ov = (row_on && e < taps) ? o[(size_t)e * ostride] : 0.f;
    const int x0 = tk.x0;
    const float t0 = ov * tk.w0, t1 = ov * tk.w1;
    const int j = __shfl(x0, lane - e) + e;                              // this lane's position
    float v = 0.f;
    bool hit = false;
#pragma unroll
    for (int q = -2; q <= 1; ++q) {                                      // taps e - 2 .. e + 1 of this row, ascending
        const int src = (lane + q) & 63;
        const int xs = __shfl(x0, src);
        const float a0 = __shfl(t0, src), a1 = __shfl(t1, src);
        const bool on = e + q >= 0 && e + q < taps;                      // (then lane + q is a lane of this row)
        if (on && xs == j) { v += a0; hit = true; }
        if (on && xs + 1 == j) { v += a1; hit = true; }
    }
    if (!row_on || !hit || j < 0 || j >= n) return;
    *entry(j) += v;
}

// over the source list: all rows of a pixel in one grid
template <int TAPS>      // TAPS = 2 * radius + 1 known at compile time (9 in every shipped config), 0 = generic
__global__ __launch_bounds__(256) void geo_lookup_bwd_acc_kernel(const MultiLookupArgs p) {
    const unsigned HW = (unsigned)p.H * p.W;
    const int taps = TAPS ? TAPS : 2 * p.radius + 1;
    const int G = taps + 2;                                              // <= 64 (host)
    const int rpw = 64 / G;                                              // rows per wave
    const unsigned nrows = (unsigned)p.B * HW * (unsigned)p.rows_per_px; // host: < 2^31
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);          // host: waves * rpw < 2^32
    const int rw = lane / G, e = lane - rw * G;
    const unsigned R = wave * (unsigned)rpw + rw;
    const bool row_on = rw < rpw && R < nrows;                           // (no early return: every lane takes part in the shuffles)
    const unsigned Rc = row_on ? R : 0u;
    const unsigned i = Rc / (unsigned)p.rows_per_px;                     // pixel
    const int j = (int)(Rc - i * (unsigned)p.rows_per_px);
    const LookupSrc s = src_of_row(p, j);
    const int c = j - s.row0;
    const unsigned b = i / HW, hw = i - b * HW;
    const float x = src_pos(s, p.disp[i], p.coords[i]);
    const float* o = s.rd + ((size_t)b * s.nch + s.ch0 + (size_t)c * taps) * HW + hw;
    acc_row_window(taps, lane, e, row_on, x, s.n, o, HW, [&](int pos) { return s.wr + ((size_t)i * s.rows + c) * s.n + pos; });
}

// over the level table: one grid slice per level, so the level is uniform and its table entries are scalar.  Written out beside the list
// form: as one body over a row finder (like the channels-last kernel) it gave the same values and its median was above the parent's range
// at 4 x 136 x 240 in three of four measurements, by up to 0.7 % (profiles/round11/lookup_one_definition.md).
template <int TAPS>
__global__ __launch_bounds__(256) void geo_lookup_level_bwd_acc_kernel(const LevelTable<float, const float> p) {
    const unsigned HW = (unsigned)p.H * p.W;
    const int taps = TAPS ? TAPS : 2 * p.radius + 1;
    const int G = taps + 2;                                              // <= 64 (host)
    const int rpw = 64 / G;                                              // rows per wave
    const unsigned nrows = (unsigned)p.B * HW * (p.C + 1);               // host: < 2^31
    const int lane = threadIdx.x & 63;
    const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);          // host: waves * rpw < 2^32
    const int l = blockIdx.y;
    const int rw = lane / G, e = lane - rw * G;
    const unsigned R = wave * (unsigned)rpw + rw;
    const bool row_on = rw < rpw && R < nrows;                           // (no early return: every lane takes part in the shuffles)
    const unsigned Rc = row_on ? R : 0u;
    const unsigned i = Rc / (unsigned)(p.C + 1);                         // pixel
    const int c = (int)(Rc - i * (unsigned)(p.C + 1));                   // row (c == C: the correlation row)
    const unsigned b = i / HW, hw = i - b * HW;
    const float scale = 1.f / (float)(1 << l);                          // exact: the dense kernels multiply 0.5f l times
    const float d = p.disp[i], cx = p.coords[i];
    const bool geo = c < p.C;
    const float x = geo ? d * scale : cx * scale - d * scale;
    const int n = geo ? p.Dl[l] : p.Wl[l];
    const int per_level = (p.C + 1) * taps;
    const float* o = p.t + (size_t)b * per_level * p.levels * HW + hw + ((size_t)l * per_level + (size_t)c * taps) * HW;
    acc_row_window(taps, lane, e, row_on, x, n, o, HW, [&](int pos) { return geo ? p.geo[l] + ((size_t)i * p.C + c) * n + pos : p.corr[l] + (size_t)i * n + pos; });
}

}  // namespace osa

using namespace osa;

extern "C" int osa_allpairs_corr_f32(const float* fmap1, const float* fmap2, float* corr,
                                     int B, int C, int H, int W1, int W2, void* stream) {
    OSA_REQUIRE(fmap1 && fmap2 && corr, "allpairs_corr: NULL pointer");
    OSA_REQUIRE(B > 0 && C > 0 && H > 0 && W1 > 0 && W2 > 0, "allpairs_corr: bad dims");
    const size_t lds = (size_t)C * 16 * sizeof(float);
    OSA_REQUIRE(lds <= 64 * 1024, "allpairs_corr: C=%d too large", C);
    const long long nblk = (long long)B * H * cdiv(W1, 16);
    hipLaunchKernelGGL(allpairs_corr_kernel, dim3((unsigned)nblk), dim3(256), lds, (hipStream_t)stream, fmap1, fmap2, corr, C, H, W1, W2);
    OSA_LAUNCH_CHECK("allpairs_corr");
    return 0;
}

extern "C" int osa_geo_rows_f32(const float* vol_ndhwc, float* rows, int B, int D, int H, int W, int C, int Cs, void* stream) {
    OSA_REQUIRE(vol_ndhwc && rows, "geo_rows: NULL pointer");
    OSA_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && C > 0 && Cs >= C, "geo_rows: bad dims");
    const size_t lds = (size_t)8 * D * (C + 1) * sizeof(float);
    OSA_REQUIRE(lds <= 160 * 1024, "geo_rows: D*C too large for LDS (%zu B)", lds);
    if (lds > 64 * 1024) (void)hipFuncSetAttribute((const void*)geo_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const long long nblk = (long long)B * H * cdiv(W, 8);
    hipLaunchKernelGGL(geo_rows_kernel, dim3((unsigned)nblk), dim3(256), lds, (hipStream_t)stream, vol_ndhwc, rows, D, H, W, C, Cs);
    OSA_LAUNCH_CHECK("geo_rows");
    return 0;
}

extern "C" int osa_avgpool_rows_f32(const float* x, float* y, long long rows, int n, void* stream) {
    OSA_REQUIRE(x && y && rows > 0 && n >= 2, "avgpool_rows: bad arguments");
    const long long total = rows * (n / 2);
    hipLaunchKernelGGL(avgpool_rows_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, rows, n);
    OSA_LAUNCH_CHECK("avgpool_rows");
    return 0;
}

// ---- the lookups' host side: one launcher for the three forms; a lookup fills its list or its level table and hands it over
namespace {
enum { LOOKUP_NCHW = 0, LOOKUP_NHWC = 1, LOOKUP_BWD = 2 };
// slices: grid slices of the accumulating form, each with rows_per_px / slices rows per pixel (the level table: one per level)
template <int FORM, class P>
int lookup_launch(const char* who, const P& a, int slices, void* stream) {
    const long long total = (long long)a.B * a.H * a.W * a.rows_per_px;    // (pixel, row) pairs
    OSA_REQUIRE(total > 0, "%s: no (pixel, row) pairs (B, H, W, C > 0)", who);
    OSA_REQUIRE(total < (1ll << 31), "%s: more than 2^31 (pixel, row) pairs", who);
    const dim3 grid((unsigned)((total + 255) / 256));
    if constexpr (FORM == LOOKUP_NCHW) {
        if constexpr (std::is_same_v<P, MultiLookupArgs>) hipLaunchKernelGGL(geo_lookup_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL(geo_lookup_level_rows_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
    } else if constexpr (FORM == LOOKUP_NHWC) {
        if (a.radius == 4) hipLaunchKernelGGL((geo_lookup_nhwc_kernel<9, P>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((geo_lookup_nhwc_kernel<0, P>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
        const int rpw = 64 / (2 * a.radius + 3);                            // rows per wave
        const long long waves = (total / slices + rpw - 1) / rpw;
        const dim3 bgrid((unsigned)((waves + 3) / 4), slices);
        if constexpr (std::is_same_v<P, MultiLookupArgs>) {
            if (a.radius == 4) hipLaunchKernelGGL(geo_lookup_bwd_acc_kernel<9>, bgrid, dim3(256), 0, (hipStream_t)stream, a);
            else hipLaunchKernelGGL(geo_lookup_bwd_acc_kernel<0>, bgrid, dim3(256), 0, (hipStream_t)stream, a);
        } else {
            if (a.radius == 4) hipLaunchKernelGGL(geo_lookup_level_bwd_acc_kernel<9>, bgrid, dim3(256), 0, (hipStream_t)stream, a);
            else hipLaunchKernelGGL(geo_lookup_level_bwd_acc_kernel<0>, bgrid, dim3(256), 0, (hipStream_t)stream, a);
        }
    }
    OSA_LAUNCH_CHECK(who);
    return 0;
}

// single pyramid.  RowT / TensorT as in LevelTable; cs: the channel stride of `t` (LOOKUP_NHWC)
template <int FORM, class RowT, class TensorT>
int pyramid_launch(const char* who, RowT* const* geo, RowT* const* corr, const int* geo_len, const int* corr_len, int levels,
                   const float* disp, const float* coords_x, TensorT* t, int cs, int B, int H, int W, int C, int radius, void* stream) {
    OSA_REQUIRE(geo && corr && geo_len && corr_len && disp && coords_x && t, "%s: NULL pointer", who);
    if (FORM == LOOKUP_BWD) OSA_REQUIRE(levels >= 1 && levels <= 4 && radius >= 0 && C >= 1, "%s: %d levels / radius %d unsupported", who, levels, radius);
    else OSA_REQUIRE(levels >= 1 && levels <= 4, "%s: %d levels unsupported (1..4)", who, levels);
    const int channels = levels * (C + 1) * (2 * radius + 1);
    if (FORM == LOOKUP_NHWC) OSA_REQUIRE(cs >= channels, "%s: channel stride %d < %d channels", who, cs, channels);
    if (FORM == LOOKUP_BWD) OSA_REQUIRE(radius <= 30, "%s: radius %d: a row's window of 2r + 3 positions has to fit a wave", who, radius);
    LevelTable<RowT, TensorT> a;
    memset(&a, 0, sizeof(a));
    for (int l = 0; l < levels; ++l) {
        OSA_REQUIRE(geo[l] && corr[l] && geo_len[l] > 0 && corr_len[l] > 0, "%s: level %d missing", who, l);
        if (FORM == LOOKUP_BWD) OSA_REQUIRE(geo_len[l] <= (1 << 19) && corr_len[l] <= (1 << 19), "%s: level %d longer than 2^19", who, l);
        a.geo[l] = geo[l]; a.corr[l] = corr[l]; a.Dl[l] = geo_len[l]; a.Wl[l] = corr_len[l];
    }
    a.disp = disp; a.coords = coords_x; a.t = t;
    a.B = B; a.H = H; a.W = W; a.C = C; a.levels = levels; a.radius = radius;
    a.rows_per_px = levels * (C + 1);
    a.nch = FORM == LOOKUP_NHWC ? cs : channels;
    return lookup_launch<FORM>(who, a, levels, stream);
}

// multi-range lookup (IGEV++): the three entry points share one argument check and one source list.
// SrcT / OutT: const float / float in the forward calls (rows read, tensors written), float / const float in the backward (rows accumulated
// into, upstream gradients read).  t[4] = geo_feat0, geo_feat1, geo_feat2, init_corr (or their gradients); cs = their channel strides (LOOKUP_NHWC).
template <int FORM, class SrcT, class OutT>
int mr_launch(const char* who, SrcT* const* g0, SrcT* const* co, const int* g0_len, const int* co_len, int levels,
              SrcT* v1, int n1, SrcT* v2, int n2, const float* disp, const float* coords_x, OutT* const t[4], const int* cs,
              int B, int H, int W, int C, int radius, void* stream) {
    OSA_REQUIRE(g0 && co && g0_len && co_len && v1 && v2 && disp && coords_x && t[0] && t[1] && t[2] && t[3], "%s: NULL pointer", who);
    OSA_REQUIRE(levels >= 1 && levels <= 4, "%s: %d levels unsupported (1..4)", who, levels);
    OSA_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && radius >= 0, "%s: bad dims", who);
    for (int l = 0; l < levels; ++l)
        OSA_REQUIRE(g0[l] && co[l] && g0_len[l] > 0 && co_len[l] > 0, "%s: level %d missing", who, l);
    OSA_REQUIRE(n1 > 0 && n2 > 0, "%s: volume 1 / 2 of length %d / %d", who, n1, n2);
    const int taps = 2 * radius + 1;
    const int count[4] = {levels * C * taps, C * taps, C * taps, levels * taps};
    if (FORM == LOOKUP_NHWC)
        for (int q = 0; q < 4; ++q) OSA_REQUIRE(cs[q] >= count[q], "%s: channel stride %d < %d channels (tensor %d)", who, cs[q], count[q], q);
    if (FORM == LOOKUP_BWD) {
        OSA_REQUIRE(radius <= 30, "%s: radius %d: a row's window of 2r + 3 positions has to fit a wave", who, radius);
        for (int l = 0; l < levels; ++l) OSA_REQUIRE(g0_len[l] <= (1 << 19) && co_len[l] <= (1 << 19), "%s: level %d longer than 2^19", who, l);
        OSA_REQUIRE(n1 <= (1 << 19) && n2 <= (1 << 19), "%s: volume 1 / 2 longer than 2^19", who);
    }
    MultiLookupArgs a;
    memset(&a, 0, sizeof(a));
    int row0 = 0;
    auto put = [&](SrcT* rows, int n, int nrows, int tensor, int ch0, float scale, int corr, bool ends_tensor) {
        LookupSrc& s = a.src[a.nsrc++];
        if constexpr (std::is_const_v<SrcT>) { s.rd = rows; s.wr = t[tensor]; } else { s.rd = t[tensor]; s.wr = rows; }
        s.n = n; s.rows = nrows; s.row0 = row0; s.ch0 = ch0; s.scale = scale; s.corr = corr;
        s.nch = FORM == LOOKUP_NHWC ? cs[tensor] : count[tensor];
        s.pad_from = ends_tensor ? count[tensor] : s.nch;
        row0 += nrows;
    };
    for (int l = 0; l < levels; ++l) put(g0[l], g0_len[l], C, 0, l * C * taps, 1.f / (float)(1 << l), 0, l == levels - 1);   // dx + disp / 2^l
    put(v1, n1, C, 1, 0, 0.5f, 0, true);                                                                                  // dx + disp / 2
    put(v2, n2, C, 2, 0, 0.25f, 0, true);                                                                                 // dx + disp / 4
    for (int l = 0; l < levels; ++l) put(co[l], co_len[l], 1, 3, l * taps, 1.f / (float)(1 << l), 1, l == levels - 1);       // coords / 2^l - disp / 2^l + dx
    a.rows_per_px = row0;
    a.disp = disp; a.coords = coords_x; a.B = B; a.H = H; a.W = W; a.radius = radius;
    return lookup_launch<FORM>(who, a, 1, stream);
}
}  // namespace

extern "C" int osa_geo_lookup_f32(const float* const* geo_levels, const float* const* corr_levels,
                                  const int* geo_len, const int* corr_len, int levels,
                                  const float* disp, const float* coords_x, float* out,
                                  int B, int H, int W, int C, int radius, void* stream) {
    return pyramid_launch<LOOKUP_NCHW>("geo_lookup", geo_levels, corr_levels, geo_len, corr_len, levels, disp, coords_x, out, 0, B, H, W, C, radius, stream);
}

extern "C" int osa_geo_lookup_nhwc_f32(const float* const* geo_levels, const float* const* corr_levels,
                                       const int* geo_len, const int* corr_len, int levels,
                                       const float* disp, const float* coords_x, float* out, int out_cs,
                                       int B, int H, int W, int C, int radius, void* stream) {
    return pyramid_launch<LOOKUP_NHWC>("geo_lookup_nhwc", geo_levels, corr_levels, geo_len, corr_len, levels, disp, coords_x, out, out_cs, B, H, W, C, radius, stream);
}

extern "C" int osa_geo_lookup_bwd_acc_f32(float* const* dgeo_levels, float* const* dcorr_levels,
                                          const int* geo_len, const int* corr_len, int levels,
                                          const float* disp, const float* coords_x, const float* dout,
                                          int B, int H, int W, int C, int radius, void* stream) {
    return pyramid_launch<LOOKUP_BWD>("geo_lookup_bwd_acc", dgeo_levels, dcorr_levels, geo_len, corr_len, levels, disp, coords_x, dout, 0, B, H, W, C, radius, stream);
}

// the dense backward has its own kernels and its own level table
extern "C" int osa_geo_lookup_bwd_f32(float* const* dgeo_levels, float* const* dcorr_levels,
                                      const int* geo_len, const int* corr_len, int levels,
                                      const float* disp, const float* coords_x, const float* dout,
                                      int B, int H, int W, int C, int radius, void* stream) {
    OSA_REQUIRE(dgeo_levels && dcorr_levels && geo_len && corr_len && disp && coords_x && dout, "geo_lookup_bwd: NULL pointer");
    OSA_REQUIRE(levels >= 1 && levels <= 4, "geo_lookup_bwd: %d levels unsupported (1..4)", levels);
    LookupBwdGatherArgs g;
    memset(&g, 0, sizeof(g));
    const long long total = (long long)B * H * W;
    long long end = 0;
    for (int l = 0; l < levels; ++l) {
        OSA_REQUIRE(dgeo_levels[l] && dcorr_levels[l] && geo_len[l] > 0 && corr_len[l] > 0, "geo_lookup_bwd: level %d missing", l);
        g.dgeo[l] = dgeo_levels[l]; g.dcorr[l] = dcorr_levels[l]; g.Dl[l] = geo_len[l]; g.Wl[l] = corr_len[l];
        end += total * C * geo_len[l]; g.seg_end[2 * l] = end;
        end += total * corr_len[l]; g.seg_end[2 * l + 1] = end;
    }
    for (int q = 2 * levels; q < 8; ++q) g.seg_end[q] = end;
    g.disp = disp; g.coords = coords_x; g.dout = dout;
    g.B = B; g.H = H; g.W = W; g.C = C; g.levels = levels; g.radius = radius;
    OSA_REQUIRE((end + 255) / 256 < (1ll << 31), "geo_lookup_bwd: grid too large");
    if (2 * radius + 1 <= 9 && (C + 1) * (2 * radius + 1) <= 256 && exp_int("OSA_GEO_BWD_FORM", 2) == 2) {     // one wave per (pixel, level): every shipped config has radius 4
        hipLaunchKernelGGL(geo_lookup_bwd_rows_kernel<9>, dim3((unsigned)((total + 3) / 4), levels), dim3(256), 0, (hipStream_t)stream, g);
        OSA_LAUNCH_CHECK("geo_lookup_bwd (rows)");
        return 0;
    }
    hipLaunchKernelGGL(geo_lookup_bwd_gather_kernel, dim3((unsigned)((end + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);   // one thread per output element
    OSA_LAUNCH_CHECK("geo_lookup_bwd (gather)");
    return 0;
}

extern "C" int osa_geo_lookup_mr_f32(const float* const* geo0_levels, const float* const* corr_levels,
                                     const int* geo0_len, const int* corr_len, int levels,
                                     const float* geo1, int geo1_len, const float* geo2, int geo2_len,
                                     const float* disp, const float* coords_x,
                                     float* geo_feat0, float* geo_feat1, float* geo_feat2, float* init_corr,
                                     int B, int H, int W, int C, int radius, void* stream) {
    float* const t[4] = {geo_feat0, geo_feat1, geo_feat2, init_corr};
    return mr_launch<LOOKUP_NCHW, const float, float>("geo_lookup_mr", geo0_levels, corr_levels, geo0_len, corr_len, levels, geo1, geo1_len, geo2, geo2_len,
                                         disp, coords_x, t, nullptr, B, H, W, C, radius, stream);
}

extern "C" int osa_geo_lookup_mr_nhwc_f32(const float* const* geo0_levels, const float* const* corr_levels,
                                          const int* geo0_len, const int* corr_len, int levels,
                                          const float* geo1, int geo1_len, const float* geo2, int geo2_len,
                                          const float* disp, const float* coords_x,
                                          float* geo_feat0, float* geo_feat1, float* geo_feat2, float* init_corr,
                                          int cs0, int cs1, int cs2, int cs_corr,
                                          int B, int H, int W, int C, int radius, void* stream) {
    float* const t[4] = {geo_feat0, geo_feat1, geo_feat2, init_corr};
    const int cs[4] = {cs0, cs1, cs2, cs_corr};
    return mr_launch<LOOKUP_NHWC, const float, float>("geo_lookup_mr_nhwc", geo0_levels, corr_levels, geo0_len, corr_len, levels, geo1, geo1_len, geo2, geo2_len,
                                         disp, coords_x, t, cs, B, H, W, C, radius, stream);
}

extern "C" int osa_geo_lookup_mr_bwd_acc_f32(float* const* dgeo0_levels, float* const* dcorr_levels,
                                             const int* geo0_len, const int* corr_len, int levels,
                                             float* dgeo1, int geo1_len, float* dgeo2, int geo2_len,
                                             const float* disp, const float* coords_x,
                                             const float* dfeat0, const float* dfeat1, const float* dfeat2, const float* dcorr_out,
                                             int B, int H, int W, int C, int radius, void* stream) {
    const float* const t[4] = {dfeat0, dfeat1, dfeat2, dcorr_out};
    return mr_launch<LOOKUP_BWD, float, const float>("geo_lookup_mr_bwd_acc", dgeo0_levels, dcorr_levels, geo0_len, corr_len, levels, dgeo1, geo1_len, dgeo2, geo2_len,
                                         disp, coords_x, t, nullptr, B, H, W, C, radius, stream);
}
