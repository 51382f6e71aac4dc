// relmc_devfn.h — device-side helper functions shared by the kernel files of librelmc.so (gfx950): DPP row moves and all-reduces over a
// scenario row, reciprocals without the IEEE division sequence, the Philox4x32-10 counter-based generator of the samplers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "relmc_dev.h"

namespace relmc {

#define DEVFI __device__ __forceinline__


template <int CTRL>
DEVFI double dppd(double v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, true); }
template <int CTRL>
DEVFI uint32_t dppu(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, true); }

// max / min as the single hardware instruction: __builtin_fmax would first canonicalise both inputs (two extra
// v_max_f64 x, x, x per call); the instruction already returns the non-NaN operand, which is the fmax semantics
DEVFI double vmax(double a, double b) { double r; __asm__("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
DEVFI double vmin(double a, double b) { double r; __asm__("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// all-reduce over the 16 lanes of a DPP row (row_ror 8,4,2,1); every lane gets bit-identical results
DEVFI double row16_sum(double v) { v += dppd<0x128>(v); v += dppd<0x124>(v); v += dppd<0x122>(v); v += dppd<0x121>(v); return v; }
DEVFI double row16_max(double v) { v = vmax(v, dppd<0x128>(v)); v = vmax(v, dppd<0x124>(v)); v = vmax(v, dppd<0x122>(v)); v = vmax(v, dppd<0x121>(v)); return v; }
DEVFI double row16_min(double v) { v = vmin(v, dppd<0x128>(v)); v = vmin(v, dppd<0x124>(v)); v = vmin(v, dppd<0x122>(v)); v = vmin(v, dppd<0x121>(v)); return v; }
DEVFI uint32_t row16_or(uint32_t v) { v |= dppu<0x128>(v); v |= dppu<0x124>(v); v |= dppu<0x122>(v); v |= dppu<0x121>(v); return v; }
DEVFI uint32_t row16_add(uint32_t v) { v += dppu<0x128>(v); v += dppu<0x124>(v); v += dppu<0x122>(v); v += dppu<0x121>(v); return v; }

// lane `l` of a wavefront as a wave-uniform (scalar) value; every lane of the wavefront must be active
DEVFI double rdlane(double v, int l)
{
    union { double d; int i[2]; } u; u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], l); u.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
    return u.d;
}
// Scenario-row all-reduces.  RW = 16: the DPP row.  RW = 64: the DPP rows first, then the four row results are
// combined in a fixed order from scalar registers (v_readlane), so the result is wave-uniform by construction.
template <int RW> DEVFI double row_sum(double v)
{
    v = row16_sum(v);
    if constexpr (RW == 64) v = (rdlane(v, 0) + rdlane(v, 16)) + (rdlane(v, 32) + rdlane(v, 48));
    return v;
}
template <int RW> DEVFI double row_max(double v)
{
    v = row16_max(v);
    if constexpr (RW == 64) v = vmax(vmax(rdlane(v, 0), rdlane(v, 16)), vmax(rdlane(v, 32), rdlane(v, 48)));
    return v;
}
template <int RW> DEVFI double row_min(double v)
{
    v = row16_min(v);
    if constexpr (RW == 64) v = vmin(vmin(rdlane(v, 0), rdlane(v, 16)), vmin(rdlane(v, 32), rdlane(v, 48)));
    return v;
}
template <int RW> DEVFI uint32_t row_or(uint32_t v)
{
    v = row16_or(v);
    if constexpr (RW == 64) v = (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) | __builtin_amdgcn_readlane((int)v, 16) | __builtin_amdgcn_readlane((int)v, 32) | __builtin_amdgcn_readlane((int)v, 48));
    return v;
}
template <int RW> DEVFI uint32_t row_add(uint32_t v)
{
    v = row16_add(v);
    if constexpr (RW == 64) v = (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) + __builtin_amdgcn_readlane((int)v, 48));
    return v;
}
template <int RW> DEVFI uint32_t row_min_u32(uint32_t v)
{
    v = min(v, dppu<0x128>(v)); v = min(v, dppu<0x124>(v)); v = min(v, dppu<0x122>(v)); v = min(v, dppu<0x121>(v));
    if constexpr (RW == 64) v = min(min((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
                                    min((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
    return v;
}
// does any lane of this scenario row hold `p`?
template <int RW> DEVFI bool row_any(bool p, int lane)
{
    const uint64_t b = __ballot(p);
    if constexpr (RW == 64) return b != 0;
    else return ((b >> (lane & 48)) & 0xffffull) != 0;
}

// 1/x to ~1 ulp (no IEEE division sequence): v_rcp_f64 is good to 4.4e-8 (measured on gfx950); with e = 1 - x r the exact reciprocal is
// r (1 + e + e^2 + ...), so ONE cubic correction r (1 + e + e^2) leaves e^3 ~ 1e-22 and a single final rounding -- three FMAs where two
// quadratic Newton steps take four (round 3: -0.6 % / -2.1 % kernel time on RTS-24 / RTS-96, results bit-identical to the two-step form)
DEVFI double frcp(double x)
{
    const double r = __builtin_amdgcn_rcp(x);
    const double e = __builtin_fma(-x, r, 1.0);
    return __builtin_fma(r, __builtin_fma(e, e, e), r);
}
// 1/a and 1/b from ONE reciprocal: R = 1/(a b), 1/a = b R, 1/b = a R (a v_rcp_f64 is quarter rate and wants its correction, two
// multiplications are cheaper; ~2 ulp instead of ~1), for the slack pair (z+, z-) and the multiplier pair (mu+, mu-) of a two-sided bound.
// Round 3 measured it per call site (profiles/r3_rcp/pair_sites.log): at ALL eight sites -1.5 % / -0.8 % kernel time on RTS-24 / RTS-96, but the
// state "G24 + G33 out" (0.3 % of all RTS-24 samples) moves from the oracle's 14 iterations to 15 -- at gamma ~ 1e-8 the Newton step of the
// static-order factorisation carries enough noise along the LP's degenerate optimal face that one more rounding cuts a dual step (alpha_d 0.57
// instead of 1, scripts/trace24.py), the extra iteration moves that state's nodal split by 6 MW on a bus and one bus' nodal sum of a sampled run
// by 2 % against the oracle.  The injection evaluation (site 1) does that on its own, the injections' ratio-test multipliers (site 5) move
// another fixture state, and combinations are not additive (0xDD and 0xD5 flip it again).  Shipped: the mask below -- line evaluation, the
// lines' ratio tests, both updates -- under which every one of the 878 + 317 fixture states keeps its iteration count and 8 of 1e6 sampled
// scenarios change theirs by one (-1.2 % kernel time).  On the 64-lane tile the same mask is 1.5 % SLOWER (the wide tile is bound by its chain, and
// the pair form is one multiplication longer) and moves which RTS-96 states the primary order fails on, which the retry tests pin: it stays at the
// round-2 arithmetic, bit for bit.  Mask 0 gives that on both tiles, 0xff all sites.
constexpr int kRpairMask = 0xCD;     // 16-lane tile.  bit 0 / 1 evaluation lines / injections, 2 / 4 ratio-test slacks (lines / injections), 3 / 5 ratio-test multipliers, 6 / 7 update lines / injections
constexpr int kInjNform = 1;         // 16-lane tile: injection evaluation with one reciprocal (of N = mu+ z- + mu- z+) instead of three
constexpr int kInjNformWide = 0;     // 64-lane tile: the same, measured -0.75 % (with the pair mask 0xCD on top -0.85 %, profiles/r3_pf/c40_v96.log); not taken: with either, one of the
                                    // 317 RTS-96 fixture states ends 6 iterations away from the C oracle (17 -> 23; the pin is +-1 on every state), tried and reverted
constexpr int kRpairMaskWide = 0;    // 64-lane tile
// The line slacks' pair reciprocal R = 1/(z+ z-) ONCE per trip (bit m = MODE m).  z+ and z- of a line change only at the very end of the update, so
// the evaluation (site 0), the ratio test (site 2) and the update (site 6) form R from the same bits; where all three are pair sites the
// evaluation keeps R in one register per line slot and the other two read it: 1/z+ = z- R, 1/z- = z+ R, the expressions and operand order of
// frcp_pair<true>, no new rounding.  The compiler cannot do it (the three sites sit under separate L_ACT regions, none dominates another).
// Not the rejected "1/z kept for both step passes" (14 doubles per lane, spilled): three doubles, lines only.  The injections share nothing:
// sites 1, 4 and 7 use three different forms.  Per mode, because the three live doubles are not free everywhere: MODE 2 (the sequential
// track) gets scratch accesses inside the interior-point loop with it and stays off.  Measurements: profiles/line_rcp_share/README.md.
#ifdef RELMC_NO_LINE_RCP_SHARE             // ablation build: every site computes its own reciprocal
constexpr int kLineRcpShareMask = 0;
#else
constexpr int kLineRcpShareMask = 0x01;      // 16-lane tile: the fused path (MODE 0 and its calibration twin)
#endif
constexpr int kLineRcpShareMaskWide = 0;   // 64-lane tile: no pair sites there (kRpairMaskWide)
template <bool PAIR>
DEVFI void frcp_pair(double a, double b, double& ra, double& rb)
{
    if constexpr (PAIR) {
        const double R = frcp(a * b);
        ra = b * R; rb = a * R;
    } else {
        ra = frcp(a); rb = frcp(b);
    }
}

// 1/x to ~2e-15 relative (measured on gfx950: raw v_rcp_f64 4.4e-8, one Newton step 2.0e-15, two steps exact):
// used where only a ratio-test bound is needed
DEVFI double frcp1(double x)
{
    const double r = __builtin_amdgcn_rcp(x);
    return __builtin_fma(r, __builtin_fma(-x, r, 1.0), r);
}
template <bool PAIR>
DEVFI void frcp1_pair(double a, double b, double& ra, double& rb)
{
    if constexpr (PAIR) {
        const double R = frcp1(a * b);
        ra = b * R; rb = a * R;
    } else {
        ra = frcp1(a); rb = frcp1(b);
    }
}

// Philox4x32-10 (Salmon et al. SC'11); counter (i_lo, i_hi, block, 0), key = seed
DEVFI void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
        c0 = n0; c1 = l1; c2 = n2; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// outage mask of the scenario (bit k = component k failed), kept in LDS behind the workspace
DEVFI bool outbit(const uint32_t* ob, int k) { return (ob[k >> 5] >> (k & 31)) & 1u; }

// a - b c with the product rounded on its own, whatever the contraction mode of the caller: the form the injection bounds are compared in
DEVFI double sub_prod(double a, double b, double c)
{
#pragma clang fp contract(off)
    return a - b * c;
}

struct __attribute__((aligned(16))) d2 { double x, y; };
DEVFI d2 ld2(const double* p) { return *reinterpret_cast<const d2*>(p); }
DEVFI void st2(double* p, double x, double y) { d2 v; v.x = x; v.y = y; *reinterpret_cast<d2*>(p) = v; }

}  // namespace relmc
