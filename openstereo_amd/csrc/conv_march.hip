// d-marching 3x3x3 convolutions (conv_march.h): instantiations and host-side launch.  A translation unit of its own so that the
// brick kernel's ~200 instantiations (conv3d.hip) are not recompiled with it.
#include "conv_march.h"
#include "conv_march_s2.h"
#include "conv_deconv_walk.h"

namespace osa {

// ------------------------------------------------------------------ d-marching form (conv_march.h) --
// 3x3x3 stride-1 "same" convolutions with 32 output channels in the f16x3 mode.  Returns 1 when launched, 0 when the layer is not
// eligible (the brick kernel then runs it), -1 on error.
static long long g_march_launches = 0;
long long march_launches() { return g_march_launches; }

struct MarchCfg { int nwv, tw, th; size_t lds; void (*fn[2][2])(const ConvArgs, int, int); };   // [split output][split input]
#define OSA_MARCH_CFG(NWV, TW) { NWV, TW, MarchGeo<NWV, TW>::TH, MarchGeo<NWV, TW>::lds_bytes(),                      \
                                 { { conv_march_kernel<NWV, TW, 0, 0>, conv_march_kernel<NWV, TW, 0, 1> },            \
                                   { conv_march_kernel<NWV, TW, 1, 0>, conv_march_kernel<NWV, TW, 1, 1> } } }
static const MarchCfg g_march_cfgs[] = {
    OSA_MARCH_CFG(4, 16),     // 0: 16 x 16 pixel column, 4 waves, 2 workgroups per CU
    OSA_MARCH_CFG(4, 32),     // 1:  8 x 32
};

int launch_conv_march(ConvArgs& a, hipStream_t st, const char* what) {
    if (!exp_int("OSA_MARCH", 1)) return 0;
    // (argument validation shared with the brick form -- check_common, check_split_ranges -- has run in conv3d_impl; what follows is
    // ELIGIBILITY: a layer this form does not cover falls through to the brick kernel, it is not an error)
    if (a.T != 27 || a.Co != 32 || a.CoP != 32 || a.Di < 3 || a.gate || a.rx) return 0;
    if (a.Ci % 16 != 0) return 0;                          // whole 16-channel chunks (the staging reads 16-channel rows, the split form is per chunk)
    const int actk = a.act & 15;
    if (actk > OSA_ACT_LEAKY || (a.act & (OSA_GATE_RAW | OSA_RES_AFTER_ACT)) || ((unsigned)a.act >> 16)) return 0;
    if ((a.yCs & 3) || ((size_t)a.y & 15) || (a.res && ((a.rCs & 3) || ((size_t)a.res & 15)))) return 0;
    if ((long long)a.Do * a.Ho * a.Wo * (a.yCs > a.rCs ? a.yCs : a.rCs) >= (1ll << 31)) return 0;
    if ((long long)a.Di * a.Hi * a.Wi * a.xCs >= (1ll << 31)) return 0;
    if (a.act & OSA_IN_SPLIT) OSA_REQUIRE(a.Ci % 16 == 0, "%s: split input needs Ci %% 16 == 0 (got %d)", what, a.Ci);
    if (a.act & OSA_OUT_SPLIT) {
        OSA_REQUIRE(a.yCs % 16 == 0, "%s: split output needs yCs %% 16 == 0", what);
        if (a.res) OSA_REQUIRE(a.act & OSA_RES_SPLIT, "%s: a split output takes a split residual", what);
    }
    if ((a.act & OSA_RES_SPLIT) && a.res) OSA_REQUIRE(a.rCs % 16 == 0, "%s: split residual needs rCs %% 16 == 0", what);
    // pixel-column shape: least padded area among the 4-wave columns (16 x 16 first: measured 2-4 % ahead of 8 x 32 at 544x960,
    // profiles/round4/march_v3_ring4_ablation_ab.txt; the 2-wave 8 x 16 column loses 20 % since the B ring costs it a workgroup per CU)
    int gi = exp_int("OSA_MARCH_GEO", -1);
    if (gi < 0 || gi > 1) {
        long long best = -1;
        for (int i = 0; i < 2; ++i) {
            const MarchCfg& g = g_march_cfgs[i];
            const long long area = (long long)cdiv(a.Ho, g.th) * g.th * cdiv(a.Wo, g.tw) * g.tw;
            if (best < 0 || area < best) { best = area; gi = i; }
        }
    }
    const MarchCfg& g = g_march_cfgs[gi];
    a.tilesD = 1; a.tilesH = cdiv(a.Ho, g.th); a.tilesW = cdiv(a.Wo, g.tw);
    a.dmin = a.hmin = a.wmin = -1;
    a.LD = 1; a.LH = g.th + 2; a.LW = g.tw + 2;
    a.VQ = 5;
    a.RowQ = (g.tw == 16) ? ((a.LW * 5 + 15) / 16 * 16) : a.LW * 5;
    a.PlaneQ = a.LH * a.RowQ;          // (one plane per pass: LD = 1; only the fp32-input variant stages through ConvArgs geometry)
    a.magicW = (unsigned)((0x100000000ull + a.LW - 1) / a.LW);
    a.magicH = (unsigned)((0x100000000ull + a.LH - 1) / a.LH);
    a.magicHW = (unsigned)((0x100000000ull + (unsigned long long)a.LH * a.LW - 1) / ((unsigned long long)a.LH * a.LW));
    a.cps = 1; a.dma = 0; a.dbg = exp_int("OSA_DBG", 0);
    // D segments: a workgroup walks dseg output planes (+ 2 boundary planes that are staged for one third of their taps).  Cost model in
    // plane-steps: rounds of resident workgroups x (dseg + 2 boundary planes of a cut column, staged and multiplied in full); the fewest segments win a tie.
    const long long cols = (long long)a.B * a.tilesH * a.tilesW;
    int per_cu = (int)((160 * 1024) / g.lds);                       // resident workgroups per CU: LDS, and 2 waves per SIMD by registers
    if (per_cu > 8 / g.nwv) per_cu = 8 / g.nwv;
    const long long slots = (long long)per_cu * 256;
    int nseg = 1;
    {
        double best = 1e30;
        for (int n = 1; n <= 16 && n * 2 <= a.Di; ++n) {
            const int ds = cdiv(a.Di, n), ns = cdiv(a.Di, ds);
            if (ns != n) continue;
            const double cost = (double)((cols * ns + slots - 1) / slots) * (ds + (ns > 1 ? 2.0 : 0.0));
            if (cost < best - 1e-9) { best = cost; nseg = ns; }
        }
        const int o = exp_int("OSA_MARCH_NSEG", 0);
        if (o > 0 && o * 2 <= a.Di) nseg = o;
    }
    const int dseg = cdiv(a.Di, nseg);
    nseg = cdiv(a.Di, dseg);
    OSA_REQUIRE(cols * nseg < (1ll << 31), "%s: grid too large", what);
    void (*fn)(const ConvArgs, int, int) = g.fn[(a.act & OSA_OUT_SPLIT) ? 1 : 0][(a.act & OSA_IN_SPLIT) ? 1 : 0];
    static bool attr_set[2][2][2];
    bool& done = attr_set[gi][(a.act & OSA_OUT_SPLIT) ? 1 : 0][(a.act & OSA_IN_SPLIT) ? 1 : 0];
    if (!done && g.lds > 64 * 1024) { (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds); }
    done = true;
    hipLaunchKernelGGL(fn, dim3((unsigned)(cols * nseg)), dim3(g.nwv * 64), g.lds, st, a, dseg, nseg);
    OSA_LAUNCH_CHECK(what);
    ++g_march_launches;
    return 1;
}

// ------------------------------------------------------------------ stride-2 d-marching form (conv_march_s2.h) --
// 3x3x3 stride-2 pad-1 convolutions with 64 output channels, f16x3 mode, split input AND split output, no residual (conv1 of the GwcNet /
// PSMNet hourglasses).  Returns 1 when launched, 0 when the layer is not eligible (the brick kernel then runs it), -1 on error.
static long long g_march_s2_launches = 0;
long long march_s2_launches() { return g_march_s2_launches; }

// osa_conv_march_s2_segment_planes: output planes per segment, 0 = the launcher's cost model (the shipped state).  A debug setter, for the
// segment-length ablation and for the tests, which pin segments that start on an odd plane and ragged last segments on small shapes.
static int g_march_s2_planes = 0;
int march_s2_planes_set(int planes) { const int prev = g_march_s2_planes; g_march_s2_planes = planes > 0 ? planes : 0; return prev; }

int launch_conv_march_s2(ConvArgs& a, hipStream_t st, const char* what) {
    if (a.T != 27 || a.Co != 64 || a.CoP != 64 || a.Di < 2 || a.gate || a.rx || a.res) return 0;
    if (a.Ci % 16 != 0 || a.xCs % 16 != 0) return 0;
    if (!(a.act & OSA_IN_SPLIT) || !(a.act & OSA_OUT_SPLIT)) return 0;
    const int actk = a.act & 15;
    if (actk > OSA_ACT_LEAKY || (a.act & (OSA_GATE_RAW | OSA_RES_AFTER_ACT)) || ((unsigned)a.act >> 16)) return 0;
    if ((a.yCs % 16) || ((size_t)a.y & 15) || ((size_t)a.x & 15)) return 0;
    if ((long long)a.Do * a.Ho * a.Wo * a.yCs >= (1ll << 31)) return 0;
    if ((long long)a.Hi * a.Wi * a.xCs >= (1ll << 29)) return 0;        // per-plane byte offsets are 32-bit
    using G = MarchS2Geo;
    a.tilesD = 1; a.tilesH = cdiv(a.Ho, G::TH); a.tilesW = cdiv(a.Wo, G::TW);
    // D segments of `oseg` output planes.  Cost model in sub-passes (one kd of one plane: 27 MFMAs per wave) per round of resident
    // workgroups: an output plane takes three, a segment that does not start at plane 0 one more (kd = 0 of the odd plane in front of it);
    // the fewest segments win a tie.
    const long long cols = (long long)a.B * a.tilesH * a.tilesW;
    const long long slots = 256;
    int nseg = 1;
    {
        double best = 1e30;
        for (int n = 1; n <= a.Do; ++n) {
            const int os = cdiv(a.Do, n), ns = cdiv(a.Do, os);
            if (ns != n) continue;
            const double cost = (double)((cols * ns + slots - 1) / slots) * (3.0 * os + (ns > 1 ? 1.0 : 0.0) + 1.5);     // (+ 1.5: prologue / drain of a workgroup)
            if (cost < best - 1e-9) { best = cost; nseg = ns; }
        }
    }
    int oseg = cdiv(a.Do, nseg);
    if (g_march_s2_planes > 0) oseg = g_march_s2_planes < a.Do ? g_march_s2_planes : a.Do;
    nseg = cdiv(a.Do, oseg);
    OSA_REQUIRE(cols * nseg < (1ll << 31), "%s: grid too large", what);
    static bool attr_set = false;                           // once per process (not inside a graph capture of a later launch)
    if (!attr_set) {
        OSA_REQUIRE(hipFuncSetAttribute((const void*)conv_march_s2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::lds_bytes()) == hipSuccess,
                    "%s: %d bytes of LDS per workgroup refused", what, (int)G::lds_bytes());
        attr_set = true;
    }
    hipLaunchKernelGGL(conv_march_s2_kernel, dim3((unsigned)(cols * nseg)), dim3(G::NWV * 64), G::lds_bytes(), st, a, oseg, nseg);
    OSA_LAUNCH_CHECK(what);
    ++g_march_s2_launches;
    return 1;
}

// ------------------------------------------------------------------ output-plane-walking transposed form (conv_deconv_walk.h) --
// 3-D stride-2 transposed convolutions k = 3 / p = 1 / op = 1 with the fused redir branch, f16x3 mode, split input, redir input and output,
// 32 or 64 output channels with as many redir channels (conv6 / conv5 of the GwcNet hourglasses).  Returns 1 when launched, 0 when the
// layer is not eligible or its class is switched off (the brick kernel then runs it), -1 on error.
static long long g_deconv_walk_launches = 0;
long long deconv_walk_launches() { return g_deconv_walk_launches; }

// osa_deconv_walk: bit 0 = the 32-output-channel class (conv6), bit 1 = the 64-output-channel class (conv5).  Defaults by measurement:
// profiles/round7/deconv_walk.md.
static int g_deconv_walk = 2;
int deconv_walk_set(int enable) { const int prev = g_deconv_walk; g_deconv_walk = enable & 3; return prev; }
// osa_deconv_walk_segment_planes: output planes per segment, 0 = the launcher's cost model (the shipped state).  A debug setter of its own, for
// the segment-length ablation and for the tests, whose small shapes the cost model would cut into one-plane segments.
static int g_deconv_walk_planes = 0;
int deconv_walk_planes_set(int planes) { const int prev = g_deconv_walk_planes; g_deconv_walk_planes = planes > 0 ? planes : 0; return prev; }

template <int WN, int RCH>
static int launch_conv_deconv_walk_t(ConvArgs& a, hipStream_t st, const char* what) {
    using G = DeconvWalkGeo<WN>;
    a.tilesD = 1; a.tilesH = cdiv(a.Hi, G::TH); a.tilesW = cdiv(a.Wi, G::TW);
    // stream index of tap (kd, kh, kw) in the class-major packed stream: class c = (pd, ph, pw) holds the taps of its parity; an even
    // parity has the one tap k = 1 (delta 0), an odd parity k = 0 (delta + 1) and k = 2 (delta 0)
    for (int t = 0, c = 0; t < a.T; ++t) {
        while (t >= a.cls_end[c]) ++c;
        const int kd = ((c >> 2) & 1) ? (a.td[t] == 1 ? 0 : 2) : 1;
        const int kh = ((c >> 1) & 1) ? (a.th[t] == 1 ? 0 : 2) : 1;
        const int kw = (c & 1) ? (a.tw[t] == 1 ? 0 : 2) : 1;
        a.toff[kd * 9 + kh * 3 + kw] = t;
    }
    // segments of `oseg` output planes (an even plane is one source plane, an odd one two; no boundary planes).  Cost model in source-plane
    // passes per round of resident workgroups (2 per CU); the fewest segments win a tie.
    const long long cols = (long long)a.B * a.tilesH * a.tilesW;
    const long long slots = 2 * 256;
    int nseg = 1;
    {
        double best = 1e30;
        for (int n = 1; n <= a.Do; ++n) {
            const int os = cdiv(a.Do, n), ns = cdiv(a.Do, os);
            if (ns != n) continue;
            const double cost = (double)((cols * ns + slots - 1) / slots) * (1.5 * os + 0.5);     // (+ 0.5: prologue / drain of a workgroup)
            if (cost < best - 1e-9) { best = cost; nseg = ns; }
        }
    }
    int oseg = cdiv(a.Do, nseg);
    if (g_deconv_walk_planes > 0) oseg = g_deconv_walk_planes < a.Do ? g_deconv_walk_planes : a.Do;
    nseg = cdiv(a.Do, oseg);
    OSA_REQUIRE(cols * nseg < (1ll << 31), "%s: grid too large", what);
    OSA_REQUIRE(hipFuncSetAttribute((const void*)conv_deconv_walk_kernel<WN, RCH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::lds_bytes()) == hipSuccess,
                "%s: %d bytes of LDS per workgroup refused", what, (int)G::lds_bytes());
    hipLaunchKernelGGL((conv_deconv_walk_kernel<WN, RCH>), dim3((unsigned)(cols * nseg)), dim3(G::NWV * 64), G::lds_bytes(), st, a, oseg, nseg);
    OSA_LAUNCH_CHECK(what);
    return 1;
}

int launch_conv_deconv_walk(ConvArgs& a, hipStream_t st, const char* what) {
    // ELIGIBILITY (argument validation has run in deconv3d_impl): anything else falls through to the brick kernel
    if (a.T != 27 || a.Do != 2 * a.Di || a.Ho != 2 * a.Hi || a.Wo != 2 * a.Wi) return 0;          // 3-D, k = 3 / p = 1 / op = 1
    if (!a.rx || a.res || a.gate) return 0;
    const int cls = (a.Co == 32 && a.rCi == 32) ? 0 : ((a.Co == 64 && a.rCi == 64) ? 1 : -1);
    if (cls < 0 || a.CoP != a.Co || !((g_deconv_walk >> cls) & 1)) return 0;
    if (!(a.act & OSA_IN_SPLIT) || !(a.act & OSA_OUT_SPLIT) || !(a.act & OSA_REDIR_SPLIT)) return 0;
    const int actk = a.act & 15;
    if (actk > OSA_ACT_LEAKY || (a.act & (OSA_GATE_RAW | OSA_RES_AFTER_ACT)) || ((unsigned)a.act >> 16)) return 0;
    if (a.Ci % 16 != 0 || a.xCs % 16 != 0 || a.yCs % 16 != 0 || a.rxCs % 16 != 0) return 0;
    if (((size_t)a.x & 15) || ((size_t)a.y & 15) || ((size_t)a.rx & 15)) return 0;
    if ((long long)a.Do * a.Ho * a.Wo * (a.yCs > a.rxCs ? a.yCs : a.rxCs) >= (1ll << 31)) return 0;
    if ((long long)a.Hi * a.Wi * a.xCs >= (1ll << 29)) return 0;        // per-plane byte offsets are 32-bit
    const int r = cls == 0 ? launch_conv_deconv_walk_t<1, 2>(a, st, what) : launch_conv_deconv_walk_t<2, 4>(a, st, what);
    if (r == 1) ++g_deconv_walk_launches;
    return r;
}

}  // namespace osa

extern "C" long long osa_conv3d_march_launches(void) { return osa::march_launches(); }
extern "C" long long osa_conv3d_march_s2_launches(void) { return osa::march_s2_launches(); }
extern "C" int osa_conv_march_s2_segment_planes(int planes) { return osa::march_s2_planes_set(planes); }
extern "C" long long osa_deconv3d_walk_launches(void) { return osa::deconv_walk_launches(); }
extern "C" int osa_deconv_walk(int enable) { return osa::deconv_walk_set(enable); }
extern "C" int osa_deconv_walk_segment_planes(int planes) { return osa::deconv_walk_planes_set(planes); }
