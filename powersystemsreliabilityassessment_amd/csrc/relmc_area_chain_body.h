// relmc_area_chain_body.h — the body of relmc_hl1_area_kernel (RELMC_AREA_TIES 0) and relmc_hl1_area_tie_kernel (RELMC_AREA_TIES 1), included
// once for each by relmc_area_kernels.h right after the kernel's signature (parameters A, load, seed, first_chain, years, start, policy,
// flow, stride, rec, and TL with ties).  Text, not a template function: as an inlined function the body compiled to a different
// schedule of the kernel without ties, which has to stay the code it was.  No include guard.
{
    constexpr bool TIES = RELMC_AREA_TIES != 0;
#if !RELMC_AREA_TIES
    const AreaTies* const TL = nullptr;                      // named in discarded statements only
#endif
    constexpr int NS = TIES ? 3 : 2;                         // cursor slots per lane: units lane, lane + 64, and tie `lane`
    constexpr int W = HL1_SEQ_WINDOW;
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int64_t cl = blockIdx.x;
    const uint64_t chain = first_chain + (uint64_t)cl;
    const int ngen = A->ngen, H = A->nhours, na = A->n_areas, nw = (ngen + 31) >> 5, nslot = ngen > 64 ? 2 : 1;
    const bool inter = policy == RELMC_HL1_AREA_INTERCONNECTED;
    double* const aE = lds + lane;                           // aE[r * 64]: this lane's EUE partial of row r in the open year ycur
    double* const mg = lds + 64 * (na + 1) + lane;
    double* const R = lds + 64 * (2 * na + 1) + lane;
    uint32_t (*const seg)[W] = reinterpret_cast<uint32_t (*)[W]>(lds + 64 * (2 * na + 1 + (inter ? na * na : 0)));
    const int64_t nsteps = (int64_t)years * H;
    double* const out = rec + (size_t)cl * (size_t)years * 3;

    bool down[NS], mine[NS];
    double tn[NS], mf[NS], mr[NS];
    int ev[NS];
    int64_t since[NS];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int k = lane + 64 * s;
        mine[s] = k < ngen;
        mf[s] = mine[s] ? A->mttf[k] : 1.0; mr[s] = mine[s] ? A->mttr[k] : 1.0;
        down[s] = false; ev[s] = 0; since[s] = 1; tn[s] = 0.0;
        if (mine[s]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[s] = hl1_seq_u(chain, k, 0, seed) < A->q[k]; ev[s] = 1; }
            tn[s] = __dmul_rn(-(down[s] ? mr[s] : mf[s]), log(hl1_seq_u(chain, k, ev[s], seed)));    // T_1 (= 0 + duration)
            ++ev[s];
        }
    }
    if constexpr (TIES) {                                    // slot 2: tie `lane`, component AREA_TIE_DRAW_BASE + lane = lane + 64 * 2
        const int k = AREA_TIE_DRAW_BASE + lane;
        mine[2] = lane < TL->n_ties && TL->mttf[lane & (AREA_TIE_MAX - 1)] < __builtin_inf();
        mf[2] = mine[2] ? TL->mttf[lane] : 1.0; mr[2] = mine[2] ? TL->mttr[lane] : 1.0;
        down[2] = false; ev[2] = 0; since[2] = 1; tn[2] = 0.0;
        if (mine[2]) {
            if (start == RELMC_HL1_START_STATIONARY) { down[2] = hl1_seq_u(chain, k, 0, seed) < TL->q[lane]; ev[2] = 1; }
            tn[2] = __dmul_rn(-(down[2] ? mr[2] : mf[2]), log(hl1_seq_u(chain, k, ev[2], seed)));
            ++ev[2];
        }
    }

    int cL[AREA_MAX + 1], cF[AREA_MAX + 1];                  // the wave's loss hours / events of the open year, per row (uniform)
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r) cL[r] = cF[r] = 0;
    for (int r = 0; r <= na; ++r) aE[r * 64] = 0.0;
    int ycur = 0, gy = 0, gh = 0;
    uint32_t prev = 0u;                                      // loss mask of the step before the group (none before step 1)
    for (int64_t w0 = 1; w0 <= nsteps; w0 += W) {
        const int64_t w1 = w0 + W;
        const int wlen = nsteps - w0 + 1 < W ? (int)(nsteps - w0 + 1) : W;
        for (int q = 0; q < nw + (TIES ? 1 : 0); ++q)
            for (int i = lane; i < W; i += 64) seg[q][i] = 0u;
        hl1_seq_wave_sync();
        // (1) down intervals [ceil(T_odd), ceil(T_even)) of the window
#pragma unroll
        for (int s = 0; s < NS; ++s) {                       // unrolled: the cursors stay in registers
            if (s < 2 && s >= nslot) { if constexpr (TIES) continue; else break; }
            bool more = mine[s];
            while (__any(more)) {
                int fb = 0, fe = 0;
                if (more) {
#if RELMC_AREA_TIES
                    // a tie may be given an MTTF far beyond any run (1e30 h): such a T has no int64 image and means "never"
                    const int64_t c = s == 2 && !(tn[s] < 9.0e18) ? INT64_MAX : (int64_t)__builtin_ceil(tn[s]);
#else
                    const int64_t c = (int64_t)__builtin_ceil(tn[s]);             // the transition takes effect from step c on
#endif
                    if (down[s]) {
                        const int64_t a = since[s] > w0 ? since[s] : w0, b = c < w1 ? c : w1;
                        if (b > a) { fb = (int)(a - w0); fe = (int)(b - w0); }
                    }
                    if (c >= w1) more = false;                                    // the cursor waits for a later window
                    else {
                        down[s] = !down[s]; since[s] = c;
                        const double l = log(hl1_seq_u(chain, lane + 64 * s, ev[s], seed));
                        tn[s] = __dadd_rn(tn[s], __dmul_rn(-(down[s] ? mr[s] : mf[s]), l));   // no FMA: the host model rounds the same way
                        ++ev[s];
                    }
                }
                for (uint64_t pend = __ballot(fe > fb); pend; pend &= pend - 1) {
                    const int src = __builtin_ctzll(pend);
                    const int sb = __builtin_amdgcn_readlane(fb, src), se = __builtin_amdgcn_readlane(fe, src), sk = src + 64 * s;
                    uint32_t* const row = seg[TIES && s == 2 ? nw : sk >> 5];
                    const uint32_t bit = 1u << (sk & 31);
                    for (int h = sb + lane; h < se; h += 64) row[h] |= bit;
                }
            }
        }
        hl1_seq_wave_sync();
        // (2) one step per lane
        for (int g = 0; g < wlen; g += 64) {
            const int i = g + lane;
            const bool valid = i < wlen;
            int h = gh + lane, y = gy;
            while (h >= H) { h -= H; ++y; }
            uint32_t fw = 0u;
            if (valid) {
                int a = 0, kend = A->lo[1];                  // area a's units end at kend (every area has one unit at least)
                double cap = 0.0;
                bool neg = false;
                for (int q = 0; q < nw; ++q) {
                    const uint32_t up = ~seg[q][i];
                    const int kn = ngen - 32 * q < 32 ? ngen - 32 * q : 32;
                    for (int b = 0; b < kn; ++b) {
                        const int k = 32 * q + b;
                        if (k == kend) {
                            const double m = cap - load[(size_t)a * H + h];
                            mg[a * 64] = m; neg |= m < 0.0;
                            cap = 0.0; ++a; kend = A->lo[a + 1];
                        }
                        cap += ((up >> b) & 1u) ? A->cap[k] : 0.0;                    // ascending units; + 0.0 is exact
                    }
                }
                const double m = cap - load[(size_t)a * H + h];
                mg[a * 64] = m; neg |= m < 0.0;
                if constexpr (TIES) {
                    if (inter && neg) {
                        const uint32_t tdown = seg[nw][i];
                        if (tdown) { area_tie_residual(R, TL, na, tdown); area_solve<false>(mg, R, nullptr, na, flow); }
                        else area_solve(mg, R, A->tie, na, flow);
                    }
                } else if (inter && neg) area_solve(mg, R, A->tie, na, flow);
#pragma unroll
                for (int r = 0; r < AREA_MAX; ++r) {
                    if (r >= na) break;
                    if (mg[r * 64] < 0.0) fw |= 1u << r;
                }
                if (fw) fw |= 1u << na;
            }
            const uint32_t fl = (uint32_t)__shfl_up((int)fw, 1);
            const uint32_t rise = fw & ~(lane == 0 ? prev : fl);
            prev = (uint32_t)__shfl((int)fw, 63);
            for (;;) {
                const bool in = valid && y == ycur;
                if (in) {
                    double ds = 0.0;
                    for (int r = 0; r < na; ++r) {
                        const double mr_ = mg[r * 64];
                        const double c = mr_ < 0.0 ? -mr_ : 0.0;
                        aE[r * 64] += c; ds += c;                // the system's deficit: sum of c_a in area order
                    }
                    aE[na * 64] += ds;
                }
#pragma unroll
                for (int r = 0; r <= AREA_MAX; ++r) {                   // a constant trip count: fully unrolled, cL / cF stay in registers
                    if (r <= na) {
                        cL[r] += (int)__popcll(__ballot(in && ((fw >> r) & 1u)));
                        cF[r] += (int)__popcll(__ballot(in && ((rise >> r) & 1u)));
                    }
                }
                if (!__any(valid && y > ycur)) break;
#pragma unroll
                for (int r = 0; r <= AREA_MAX; ++r)
                    if (r <= na) area_close_year(aE[r * 64], cL[r], cF[r], out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3);
                ++ycur;
            }
            gh += 64;
            while (gh >= H) { gh -= H; ++gy; }
        }
        hl1_seq_wave_sync();
    }
#pragma unroll
    for (int r = 0; r <= AREA_MAX; ++r)
        if (r <= na) area_close_year(aE[r * 64], cL[r], cF[r], out + (size_t)r * (size_t)stride * 3 + (size_t)ycur * 3);
}
