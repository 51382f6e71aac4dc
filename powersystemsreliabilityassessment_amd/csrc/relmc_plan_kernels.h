// relmc_plan_kernels.h — kernels of the HL1 planning model's Monte Carlo (generating_adequancy_comparative.jl:15-120, tail_risk.jl:12-91):
// planned maintenance, energy-limited units (ELUs) and load forecast uncertainty.  Contract in include/relmc.h.
#pragma once
#include "relmc_devfn.h"

namespace relmc {

// Unit k's contribution to the hour: skipped in maintenance or down; an ELU adds to cap_elu unless exhausted (bit of `exh`)
DEVFI void plan_unit(const PlanUnit& u, int h, uint32_t w, uint32_t exh, double& cap_unl, double& cap_elu, uint32_t& avail)
{
    if (h >= u.mlo && h < u.mhi) return;             // wave-uniform
    if (w < u.thr) return;
    if (u.slot < 0) cap_unl += u.cap;                // ascending unit order
    else if (!((exh >> u.slot) & 1u)) { cap_elu += u.cap; avail |= 1u << u.slot; }
}

// One lane per year: all lanes of a wavefront step through the same hour, so the load and every unit's record are scalar loads; the
// ELU energies and the loss flag stay in registers (ELU slots are addressed through bit masks and unrolled loops, never a run-time
// register index).  The per-hour loss count is ballot + popcount, added by lane 0 with a 64-bit integer atomic when nonzero.
// Records: year_out[year][3] = (loss hours, EUE, loss events), summed by relmc_hl1_reduce_kernel (relmc_seq_kernels.h);
// elu_out[year][n_elu] (optional).
__global__ void __launch_bounds__(256) relmc_hl1_plan_kernel(const PlanCase* __restrict__ P, const double* __restrict__ load, uint64_t seed,
                                                             uint64_t first_year, int64_t n_years, double* __restrict__ year_out,
                                                             double* __restrict__ elu_out, unsigned long long* __restrict__ hour_count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63) >= n_years) return;     // wave-uniform: the wave has no year
    const bool valid = i < n_years;
    const uint64_t y = first_year + (uint64_t)(valid ? i : 0);
    const uint32_t y0 = (uint32_t)y, y1 = (uint32_t)(y >> 32), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const int ngen = P->ngen, H = P->nhours, nblk = P->nblk, nelu = P->n_elu;
    const double sigma = P->sigma;
    double en[PLAN_MAX_ELU];
#pragma unroll
    for (int e = 0; e < PLAN_MAX_ELU; ++e) en[e] = 0.0;
    double aL = 0.0, aE = 0.0, aF = 0.0;
    bool prev = false;
    for (int h = 0; h < H; ++h) {
        uint32_t exh = 0;
#pragma unroll
        for (int e = 0; e < PLAN_MAX_ELU; ++e) exh |= (en[e] >= P->elu_lim[e] ? 1u : 0u) << e;
        double cap_unl = 0.0, cap_elu = 0.0;
        uint32_t avail = 0;
        uint32_t w[4];
        const uint32_t c2 = PLAN_TAG | (uint32_t)h;
        philox4x32_10(y0, y1, c2, 0u, k0, k1, w);
        const double u1 = ((double)w[0] + 0.5) * 2.3283064365386963e-10, u2 = ((double)w[1] + 0.5) * 2.3283064365386963e-10;
        const double z = __dmul_rn(sqrt(__dmul_rn(-2.0, log(u1))), cos(__dmul_rn(6.283185307179586, u2)));
        if (ngen > 0) plan_unit(P->unit[0], h, w[2], exh, cap_unl, cap_elu, avail);
        if (ngen > 1) plan_unit(P->unit[1], h, w[3], exh, cap_unl, cap_elu, avail);
        for (int b = 1; b < nblk; ++b) {
            philox4x32_10(y0, y1, c2, (uint32_t)b, k0, k1, w);
            const int kb = 4 * b - 2;
#pragma unroll
            for (int j = 0; j < 4; ++j)                                            // j unrolled: w[j] is a register, not an index
                if (kb + j < ngen) plan_unit(P->unit[kb + j], h, w[j], exh, cap_unl, cap_elu, avail);
        }
        const double ld = __dadd_rn(load[h], __dmul_rn(z, sigma));
        const double x = ld - cap_unl;
        const double uns = x > 0.0 ? x : 0.0;
        const bool f = uns > cap_elu;
        const double d = f ? uns - cap_elu : 0.0;
        if (f) {
#pragma unroll
            for (int e = 0; e < PLAN_MAX_ELU; ++e)
                if ((avail >> e) & 1u) en[e] += P->elu_cap[e];
        } else if (uns > 0.0) {
#pragma unroll
            for (int e = 0; e < PLAN_MAX_ELU; ++e)
                if ((avail >> e) & 1u) en[e] = __dadd_rn(en[e], __dmul_rn(uns, P->elu_cap[e] / cap_elu));
        }
        aL += f ? 1.0 : 0.0;
        aE += d;
        aF += (f && !prev) ? 1.0 : 0.0;
        prev = f;
        const uint64_t m = __ballot(valid && f);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(hour_count + h, (unsigned long long)__popcll(m));
    }
    if (!valid) return;
    year_out[3 * i] = aL; year_out[3 * i + 1] = aE; year_out[3 * i + 2] = aF;
    if (elu_out) {
#pragma unroll
        for (int e = 0; e < PLAN_MAX_ELU; ++e)
            if (e < nelu) elu_out[(size_t)i * nelu + e] = en[e];
    }
}

}  // namespace relmc
