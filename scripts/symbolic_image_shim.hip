// symbolic_image_shim.hip — the whole device image of a case as case_symbolic writes it, for byte-for-byte comparisons of two builds of
// csrc/relmc_schedule.hip (scripts/symbolic_ab.py; profiles/symbolic_steps/README.md).  Not part of librelmc.so: link it with that one unit,
//   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -shared -I<csrc> <csrc>/relmc_schedule.hip scripts/symbolic_image_shim.hip -o shim.so
// With -DSHIM_MAIN it is a program of its own (ring networks with chords on both tiles), which is what a host sanitizer build runs.
#include <cstring>
#include <memory>

#include "relmc_ctx.h"

using namespace relmc_host;

// opts[9]: no_quarter, no_half, no_bwd_half, no_bus_map, place_moves, place_ww, scen_pad4, model_leaf_free, unused (negative = the default)
// geom[8]: stash_off, scen_doubles, lds_bytes, conflict_before, conflict_after, shadow_masked, shadow_tasks, shadow_all
extern "C" int32_t symbolic_image(const relmc_case_desc* d, int32_t variant, const int32_t* hint, int32_t n_hint, const int64_t* opts, uint8_t* image,
                                  int64_t image_cap, int64_t* image_bytes, int64_t* geom, char* err, int32_t err_cap)
{
    SymOpts so = sym_opts_default();
    if (hint && n_hint > 0) { so.order_hint = hint; so.n_hint = n_hint; }
    so.no_quarter = opts[0] > 0; so.no_half = opts[1] > 0; so.no_bwd_half = opts[2] > 0; so.no_bus_map = opts[3] > 0;
    if (opts[4] >= 0) so.place_moves = (int)opts[4];
    if (opts[5] >= 0) so.place_ww = (long)opts[5];
    if (opts[6] >= 0) so.scen_pad4 = (int)opts[6];
    if (opts[7] >= 0) so.model_leaf_free = (int)opts[7];
    SymGeom g;
    std::string errs;
    int rc;
    auto run = [&](auto tile) {
        using TL = decltype(tile);
        auto C = std::make_unique<DevCaseT<TL>>();
        std::memset(C.get(), 0, sizeof(*C));
        const int r = case_symbolic<TL>(d, *C, variant, so, g, errs);
        *image_bytes = (int64_t)sizeof(*C);
        if ((int64_t)sizeof(*C) <= image_cap) std::memcpy(image, C.get(), sizeof(*C));
        return r;
    };
    rc = fits_tile24(d) ? run(Tile24{}) : run(Tile96{});
    const long gv[8] = {(long)g.stash_off, (long)g.scen_doubles, (long)g.lds_bytes, g.conflict_before, g.conflict_after, g.shadow_masked, g.shadow_tasks, g.shadow_all};
    for (int k = 0; k < 8; ++k) geom[k] = gv[k];
    if (err && err_cap > 0) { std::strncpy(err, errs.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return rc;
}

#ifdef SHIM_MAIN
#include <cstdio>
// a ring of nb buses with a chord every `step` buses, one generator and one load per third bus: sizes on both tiles and one past the wide one
static int ring(int nb, int step)
{
    std::vector<int32_t> from, to, inj_bus;
    for (int i = 0; i < nb; ++i) { from.push_back(i); to.push_back((i + 1) % nb); }
    for (int i = 0; i + step < nb && (int)from.size() < 120; i += step) if (step > 1) { from.push_back(i); to.push_back(i + step); }
    const int nl = (int)from.size();
    for (int i = 0; i < nb; i += 3) inj_bus.push_back(i);
    const int ng = (int)inj_bus.size();
    for (int i = 1; i < nb; i += 3) inj_bus.push_back(i);
    const int nd = (int)inj_bus.size() - ng, ninj = ng + nd;
    std::vector<double> pd(nb, 1.0), pmin(ninj, 0.0), pmax(ninj, 50.0), cost(ninj, 1.0), b(nl, 10.0), rate(nl, 100.0), un(ng + nl, 0.02);
    std::vector<uint8_t> up(ng + nl, 0);
    relmc_case_desc d = {};
    d.base_mva = 100.0; d.nb = nb; d.ng = ng; d.nl = nl; d.nd = nd; d.ref_bus = 0; d.total_load = nb;
    d.bus_pd = pd.data(); d.inj_bus = inj_bus.data(); d.inj_pmin = pmin.data(); d.inj_pmax = pmax.data(); d.inj_cost = cost.data();
    d.br_from = from.data(); d.br_to = to.data(); d.br_b = b.data(); d.br_rate = rate.data(); d.unavail = un.data(); d.always_up = up.data();
    std::vector<uint8_t> image(sizeof(DevCaseT<Tile96>) > sizeof(DevCaseT<Tile24>) ? sizeof(DevCaseT<Tile96>) : sizeof(DevCaseT<Tile24>));
    int worst = 0;
    for (int variant = 0; variant < 3; ++variant) {
        const int64_t opts[9] = {0, 0, 0, 0, -1, -1, -1, -1, -1};
        int64_t bytes = 0, geom[8]; char err[256];
        const int rc = symbolic_image(&d, variant, nullptr, 0, opts, image.data(), (int64_t)image.size(), &bytes, geom, err, 256);
        unsigned long sum = 0;
        for (int64_t k = 0; k < bytes; ++k) sum = sum * 31 + image[(size_t)k];
        std::printf("ring nb=%d step=%d variant=%d: rc=%d bytes=%ld checksum=%lx lds=%ld %s\n", nb, step, variant, rc, (long)bytes, sum, (long)geom[2], err);
        if (rc != RELMC_OK && rc != RELMC_ERR_UNSUPPORTED) worst = 1;
    }
    return worst;
}
int main() { return ring(12, 5) | ring(24, 7) | ring(90, 11) | ring(140, 9); }
#endif
