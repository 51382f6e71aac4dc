// relmc_debug.hip — introspection and test hooks that are not part of include/relmc.h (bound by the Python test suite and the profiling
// scripts through ctypes): the active schedule's shape, every Newton step through the dense pivoted solve, per-phase cycle counters and
// per-iteration traces of the profiling builds, the stretch-length rule of relmc_nsq_run, the dynamic tail's plan, the diagnosis switches of a
// context.
#include <cstdio>
#include <cstring>
#include <memory>

#include "relmc_ctx.h"
#include "relmc_shape_rts24.h"

using namespace relmc_host;

extern "C" {

// introspection: {npass_upd, npass_inv, npass_bwd, noff, nzero, nws, lds_bytes, blocks_per_cu, total tasks}
int32_t relmc_debug_schedule(const relmc_ctx* ctx, int32_t* out9)
{
    if (!ctx || !out9 || !ctx->has_case) return RELMC_ERR_INVALID;
    auto fill = [&](const auto& C) {
        int ntask = 0;
        for (int p = 0; p < C.npass; ++p) ntask += C.pass_ntask[p];
        out9[0] = C.npass_upd; out9[1] = C.npass_inv; out9[2] = C.npass - C.npass_upd - C.npass_inv; out9[3] = C.noff;
        out9[4] = C.nzero; out9[5] = (int)C.nws; out9[6] = (int)ctx->lds_bytes; out9[7] = ctx->blocks_per_cu; out9[8] = ntask;
        if (verbose()) fprintf(stderr, "relmc: modelled LDS conflict cycles per Newton step %ld -> %ld\n", ctx->conflict_before, ctx->conflict_after);
        if (verbose()) fprintf(stderr, "relmc: longest line / injection list per bus slot: %d %d / %d %d\n", (int)C.maxdeg_s[0], (int)C.maxdeg_s[1], (int)C.maxinj_s[0], (int)C.maxinj_s[1]);
        if (verbose()) { fprintf(stderr, "relmc: tasks per pass:"); for (int p = 0; p < C.npass; ++p) fprintf(stderr, " %d", (int)C.pass_ntask[p]); fprintf(stderr, "\n"); }
    };
    if (ctx->tile == 0) fill(ctx->hcase24); else fill(ctx->hcase96);
    return RELMC_OK;
}

// test hook: mc_simulation with EVERY Newton step solved by the dense, partially pivoted last resort (MODE 6) instead of the static
// sparse schedule -- tests/test_gpu_parity.py compares it with the shipped solver and with the C oracle (whose LU pivots as well)
int32_t relmc_debug_mc_simulation_dense(relmc_ctx* ctx, const uint8_t* states_host, int64_t n, const relmc_solver_opts* opts, double* dns_host,
                                        double* nodal_host, int32_t* status_host, int32_t* iters_host)
{
    if (!ctx || !ctx->has_case || !states_host || !dns_host || n < 0) return RELMC_ERR_INVALID;
    if (n == 0) return RELMC_OK;
    const relmc_solver_opts o = solver_opts_or_default(opts);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int ow = mask_words(ctx), ncomp = ctx->ncomp, nb = ctx->nb;
    std::vector<uint32_t> keys((size_t)n * ow, 0u);
    for (int64_t r = 0; r < n; ++r) for (int k = 0; k < ncomp; ++k) if (states_host[(size_t)r * ncomp + k]) keys[(size_t)r * ow + (k >> 5)] |= 1u << (k & 31);
    DevBuf<uint32_t> dk; DevBuf<double> dd, dn; DevBuf<int32_t> dm;
    if (dk.grow(keys.size()) != hipSuccess || dd.grow((size_t)n) != hipSuccess || dm.grow((size_t)n) != hipSuccess || dn.grow((size_t)n * nb) != hipSuccess)
        return fail(ctx, RELMC_ERR_HIP, "dense simulation: device allocation failed");
    int rc = RELMC_OK;
    if (hipMemcpy(dk.get(), keys.data(), sizeof(uint32_t) * keys.size(), hipMemcpyHostToDevice) != hipSuccess) rc = fail(ctx, RELMC_ERR_HIP, "dense simulation: H2D failed");
    EvalArgs a = make_args(o);
    a.n = n; a.memo_keys = dk.get(); a.db_first = 0; a.dns = dd.get(); a.status = dm.get(); a.nodal = dn.get();
    int rows = 0;
    if (rc == RELMC_OK) rc = launch_eval(ctx, 6, a, &rows);
    if (rc == RELMC_OK) rc = finish_timing(ctx);
    std::vector<int32_t> meta((size_t)n);
    if (rc == RELMC_OK && (hipMemcpy(dns_host, dd.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
                           hipMemcpy(meta.data(), dm.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
                           (nodal_host && hipMemcpy(nodal_host, dn.get(), sizeof(double) * (size_t)n * nb, hipMemcpyDeviceToHost) != hipSuccess)))
        rc = fail(ctx, RELMC_ERR_HIP, "dense simulation: D2H failed");
    if (rc) return rc;
    for (int64_t r = 0; r < n; ++r) { if (status_host) status_host[r] = meta[(size_t)r] & 3; if (iters_host) iters_host[r] = (int32_t)((uint32_t)meta[(size_t)r] >> 8); }
    return RELMC_OK;
}

// profiling hook (only meaningful in -DRELMC_PHASE_TIMING builds): per-phase cycle sums of the last launch
int32_t relmc_debug_phase_cycles(relmc_ctx* ctx, unsigned long long* out8)
{
    if (!ctx || !out8) return RELMC_ERR_INVALID;
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    if (!ctx->dtiming.get() || ctx->timing_waves <= 0) return RELMC_OK;
    std::vector<unsigned long long> h((size_t)ctx->timing_waves * 8);
    HIP_TRY(ctx, hipMemcpy(h.data(), ctx->dtiming.get(), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int w = 0; w < ctx->timing_waves; ++w) for (int k = 0; k < 8; ++k) out8[k] += h[(size_t)w * 8 + k];
    return RELMC_OK;
}

// profiling hook (only meaningful in -DRELMC_PHASE_TIMING builds): the last launch's trips of the interior-point loop, summed over its wavefronts,
// by the form of their evaluation: out2[0] without the second-stage termination norms, out2[1] with them
int32_t relmc_debug_norm_trips(relmc_ctx* ctx, unsigned long long* out2)
{
    if (!ctx || !out2) return RELMC_ERR_INVALID;
    out2[0] = out2[1] = 0;
    if (!ctx->dtiming.get() || ctx->timing_waves <= 0) return RELMC_OK;
    std::vector<unsigned long long> h((size_t)ctx->timing_waves * 2);
    HIP_TRY(ctx, hipMemcpy(h.data(), ctx->dtiming.get() + (size_t)ctx->timing_waves * 8, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int w = 0; w < ctx->timing_waves; ++w) for (int k = 0; k < 2; ++k) out2[k] += h[(size_t)w * 2 + k];
    return RELMC_OK;
}

// debug hook (only meaningful in -DRELMC_TRACE builds): per-iteration termination quantities of the first scenario
// of the last launch, 8 doubles per iteration {feascond, gradcond, compcond, costcond, alpha_p, alpha_d, gamma, f}
int32_t relmc_debug_trace(relmc_ctx* ctx, double* out, int32_t n_doubles)
{
    if (!ctx || !out || n_doubles < 0) return RELMC_ERR_INVALID;
    for (int k = 0; k < n_doubles; ++k) out[k] = 0.0;
    if (!ctx->dtiming.get() || n_doubles > 8 * 65536) return RELMC_OK;
    HIP_TRY(ctx, hipMemcpy(out, ctx->dtiming.get(), sizeof(double) * n_doubles, hipMemcpyDeviceToHost));
    return RELMC_OK;
}

// The shape fields of relmc_shape.h (SF_COUNT values, in ShapeField order).  case_out: what relmc_case_load computes for this case under the
// given primary order (host only: no device, no context; null = skip); static_out: the shape compiled into the specialised fused kernel
// (relmc_shape_rts24.h; null = skip).  Returns the number of fields, or a negative error.
int32_t relmc_debug_shape(const relmc_case_desc* d, const int32_t* order_hint, int32_t n_hint, int32_t* case_out, int32_t* static_out)
{
    int32_t v[SF_COUNT_ALL];          // the fill-lane fields behind SF_COUNT are relmc_debug_fill_lanes'
    if (static_out) { ShapeRts24::values(v); std::memcpy(static_out, v, sizeof(int32_t) * SF_COUNT); }
    if (case_out) {
        if (!d) return RELMC_ERR_INVALID;
        SymOpts so = sym_opts_default();
        if (order_hint && n_hint > 0) { so.order_hint = order_hint; so.n_hint = n_hint; }
        std::string err;
        SymGeom g;
        const int rc = with_symbolic(d, 0, so, g, err, [&](const auto& C) { shape_of(C, g.stash_off, g.scen_doubles, v); return (int)RELMC_OK; });
        if (rc) return rc < 0 ? rc : -rc;
        std::memcpy(case_out, v, sizeof(int32_t) * SF_COUNT);
    }
    return SF_COUNT;
}

// Host-only introspection: which lane clears which fill block (relmc_dev.h: l_blk_fill, b_lane_fill), for the case / order arguments of
// relmc_debug_symbolic.
//   hdr[17]: RW, nb, nl, nzero, nzero_res, nfill_line, nfill_bus, line-slot lanes of the tile (NLT), bus-slot lanes (NBT), the compiled-in
//            shape's nzero_res and nfill_bus (relmc_shape_rts24.h; relmc_debug_shape keeps to the fields in front of them), nidle_line,
//            nidle_bus_s[0], nidle_bus_s[1], and the compiled-in shape's three
//   l_blk_fill[NLT], b_lane_fill[NBT], b_lane[NBT] (null = skip): the tables as the device gets them
int32_t relmc_debug_fill_lanes(const relmc_case_desc* d, int32_t order_variant, const int32_t* order_hint, int32_t n_hint, int32_t* hdr, uint16_t* l_blk_fill,
                               uint16_t* b_lane_fill, uint8_t* b_lane)
{
    if (!d || !hdr) return RELMC_ERR_INVALID;
    SymOpts so = sym_opts_default();
    if (order_hint && n_hint > 0) { so.order_hint = order_hint; so.n_hint = n_hint; }
    std::string err;
    SymGeom g;
    return with_symbolic(d, order_variant, so, g, err, [&](const auto& C) {
        using DC = std::decay_t<decltype(C)>;
        int32_t st[SF_COUNT_ALL];
        ShapeRts24::values(st);
        hdr[0] = DC::ROWL; hdr[1] = C.nb; hdr[2] = C.nl; hdr[3] = C.nzero; hdr[4] = C.nzero_res; hdr[5] = C.nfill_line; hdr[6] = C.nfill_bus; hdr[7] = DC::NLT; hdr[8] = DC::NBT;
        hdr[9] = st[SF_NZERO_RES]; hdr[10] = st[SF_NFILL_BUS];
        hdr[11] = C.nidle_line; hdr[12] = C.nidle_bus_s[0]; hdr[13] = C.nidle_bus_s[1]; hdr[14] = st[SF_NIDLE_LINE]; hdr[15] = st[SF_NIDLE_BUS0]; hdr[16] = st[SF_NIDLE_BUS1];
        for (int l = 0; l < DC::NLT; ++l) if (l_blk_fill) l_blk_fill[l] = C.l_blk_fill[l];
        for (int q = 0; q < DC::NBT; ++q) { if (b_lane_fill) b_lane_fill[q] = C.b_lane_fill[q]; if (b_lane) b_lane[q] = C.b_lane[q]; }
        return (int)RELMC_OK;
    });
}

// relmc_nsq_run's stretch-length rule (stretch_length, relmc_nsq_run.hip; host only) with the library's own longest stretch for this batch:
// the length of the stretch after `done` samples at `beta`, *final_out (optional) = 1 if it is sized to end the run; negative = bad arguments
int64_t relmc_debug_stretch_len(int64_t batch, int64_t done, double beta, double beta_limit, int64_t round, int32_t* final_out)
{
    if (batch <= 0 || batch > kStretchMaxBatch || done < 0 || round < 0) return RELMC_ERR_INVALID;
    const Stretch s = stretch_length(batch, done, beta, beta_limit, stretch_per(batch), round);
    if (final_out) *final_out = s.final ? 1 : 0;
    return s.len;
}

// which evaluation kernel the fused path of this context launches now: 1 = the shape-specialised instantiation, 0 = the run-time-shape one
int32_t relmc_debug_shape_path(const relmc_ctx* ctx)
{
    if (!ctx || !ctx->has_case) return RELMC_ERR_INVALID;
    return ctx->shape_static && !ctx->sw.dynamic_shape ? 1 : 0;
}

// The dynamic tail's plan for a fused launch of n scenarios on `waves` wavefronts of the 16-lane tile (TailPlan, relmc_ctx.h; host only: no
// device, no context).  Returns T.  Optional outputs: a_begin / a_end [waves] = every wavefront's phase-A range of groups, owner / group
// [waves * T] = the wavefront that owns item p of the claim counter and the group the item stands for; negative = bad arguments.
int32_t relmc_debug_tail_plan(int64_t n, int32_t waves, int64_t* a_begin, int64_t* a_end, int32_t* owner, int64_t* group)
{
    if (n < 0 || waves <= 0) return RELMC_ERR_INVALID;
    const TailPlan plan(n, waves);
    for (int64_t w = 0; w < waves; ++w) { if (a_begin) a_begin[w] = plan.begin(w); if (a_end) a_end[w] = plan.cut(w); }
    for (int64_t p = 0; p < plan.items(); ++p) { if (owner) owner[p] = (int32_t)plan.owner(p); if (group) group[p] = plan.group(p); }
    return plan.T;
}

// T of the context's last fused launch on the 16-lane tile (what RELMC_VERBOSE prints per launch): 0 = it ran without the dynamic tail;
// *launches_out (optional) = the fused launches of the context that ran with one so far; *waves_out (optional) = the wavefronts of a full
// grid of the 16-lane tile on this device (CUs x workgroups per CU x 4), 0 before a case is loaded
int32_t relmc_debug_tail_groups(const relmc_ctx* ctx, int64_t* launches_out, int32_t* waves_out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (launches_out) *launches_out = ctx->tail_launches;
    if (waves_out) *waves_out = ctx->has_case && ctx->tile == 0 ? ctx->num_cu * ctx->blocks_per_cu * Tile24::WPB : 0;
    return ctx->last_tail_groups;
}

// test hook: the event kernels of relmc_seq_events (count -> offsets -> fill -> reduce, seq_events_device of relmc_seq.hip) on caller-given
// hours curt[n_years][hpy] and masks[n_years][hpy][mw] (mw 32-bit words per hour, bit k of word k / 32 = component k down) instead of a
// relmc_seq_years step's.  Needs a context but no case.  hpy 1..65535 and mw 1..8, the chronology kernel's limits; the other arguments as
// relmc_seq_events.
int32_t relmc_debug_seq_events(relmc_ctx* ctx, int32_t n_years, int32_t hpy, int32_t mw, const double* curt_host, const uint32_t* masks_host,
                               double curtail_threshold, relmc_seq_event_acc* ev_acc, int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap,
                               relmc_seq_event* events_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (n_years < 0 || hpy < 1 || hpy > 65535 || mw < 1 || mw > SEQ_EVENT_MW || !ev_acc || (n_years > 0 && (!curt_host || !masks_host)) ||
        (dur_hist_host && (n_dur_bins < 1 || n_dur_bins > 4096)) || events_cap < 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_debug_seq_events: bad arguments");
    seq_events_zero(ev_acc, n_dur_bins, dur_hist_host);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t nh = (size_t)n_years * hpy;
    DevBuf<double> dc; DevBuf<uint32_t> dm;
    if (nh > 0) {
        HIP_TRY(ctx, dc.grow(nh));
        HIP_TRY(ctx, dm.grow(nh * mw));
        HIP_TRY(ctx, hipMemcpy(dc.get(), curt_host, sizeof(double) * nh, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(dm.get(), masks_host, sizeof(uint32_t) * nh * mw, hipMemcpyHostToDevice));
    }
    double ms = 0.0;
    const int rc = seq_events_device(ctx, "relmc_debug_seq_events", dc.get(), dm.get(), n_years, hpy, mw, curtail_threshold, -1, ev_acc, n_dur_bins,
                                     dur_hist_host, events_cap, events_host, &ms);
    ctx->last_kernel_ms = ms;
    return rc;
}

// diagnosis switches of the context (tests): "no_retry", "retry_dense_first", "nsq_no_stretch", "db_no_probe", "dynamic_shape", "static_tail",
// "norms_always"; value 0 / 1.  static_tail may change between launches: the fused path then runs without the dynamic tail (tests/test_tail_paths.py).
// no_retry must be set before relmc_case_load (the order calibration and the list arming must agree).  dynamic_shape may change between
// launches: the fused path then runs the run-time-shape kernel on a case that has the compiled-in shape (tests/test_shape_paths.py).
// norms_always may change between launches: every evaluation kernel then accumulates the second-stage termination norms on every trip of the
// interior-point loop instead of only on the trips that can end; same results bit for bit (tests/test_norm_paths.py).
int32_t relmc_debug_set(relmc_ctx* ctx, const char* key, int32_t value)
{
    if (!ctx || !key) return RELMC_ERR_INVALID;
    const bool v = value != 0;
    if (!std::strcmp(key, "no_retry")) ctx->sw.no_retry = v;
    else if (!std::strcmp(key, "retry_dense_first")) ctx->sw.retry_dense_first = v;
    else if (!std::strcmp(key, "nsq_no_stretch")) ctx->sw.nsq_no_stretch = v;
    else if (!std::strcmp(key, "db_no_probe")) ctx->sw.db_no_probe = v;
    else if (!std::strcmp(key, "dynamic_shape")) ctx->sw.dynamic_shape = v;
    else if (!std::strcmp(key, "static_tail")) ctx->sw.static_tail = v;
    else if (!std::strcmp(key, "norms_always")) ctx->sw.norms_always = v;
    else return fail(ctx, RELMC_ERR_INVALID, std::string("relmc_debug_set: unknown switch ") + key);
    return RELMC_OK;
}

}  // extern "C"
