// relmc_schedule.hip — symbolic analysis of a study case and the static solver schedule the evaluation kernel interprets (host arithmetic
// only: no HIP call, no context), plus the offline tuner of the primary elimination order.  What nsqMain.m:42-167 prepares once before
// its Monte Carlo loop; MATLAB's `\` under MIPS picks its own pivot order per call (mc_simulation.m:41), here the order is fixed per case.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "relmc_ctx.h"
#ifdef RELMC_DEV_SWITCHES
#include "relmc_dev_switches.h"
#endif

namespace relmc_host {

bool verbose()
{
    static const bool v = std::getenv("RELMC_VERBOSE") != nullptr;      // the library's only environment variable in the default build
    return v;
}

SymOpts sym_opts_default()
{
    SymOpts so;
#ifdef RELMC_DEV_SWITCHES      // ablation builds (csrc/Makefile: ablate/librelmc_dev.so): schedule forms and search weights from the environment
    relmc_dev_switches_schedule(so);
#endif
    return so;
}

namespace {

// ---- the LDS bank model.  ds_read_b128 serves a wavefront in four fixed 16-lane groups (MI355X_MICROARCH.md), bank = (byte address / 4)
// mod 64: a group is conflict-free when its 16 lanes hit 16 different 16-byte bank slots; equal addresses are one broadcast.
const int kGroupOfLane[64] = {0,0,0,0,1,1,1,1,1,1,1,1,0,0,0,0, 1,1,1,1,0,0,0,0,0,0,0,0,1,1,1,1,
                              2,2,2,2,3,3,3,3,3,3,3,3,2,2,2,2, 3,3,3,3,2,2,2,2,2,2,2,2,3,3,3,3};
struct BankCount {                           // the conflicts of ONE LDS instruction: the byte address of every lane that takes part goes in
    int cnt[4][16] = {}; int addr[4][16][16];
    void add(int lane, int ad)
    {
        const int g = kGroupOfLane[lane], q = (ad >> 4) & 15;
        for (int k = 0; k < cnt[g][q]; ++k) if (addr[g][q][k] == ad) return;
        addr[g][q][cnt[g][q]++] = ad;
    }
    long extra() const                       // extra cycles: per group, the most different addresses in one bank slot, minus one
    {
        long c = 0;
        for (int g = 0; g < 4; ++g) { int mx = 0; for (int q = 0; q < 16; ++q) if (cnt[g][q] > mx) mx = cnt[g][q]; if (mx > 1) c += mx - 1; }
        return c;
    }
};
// operand reads per pass form as (descriptor field, byte offset); the full form's last two are the second row (not read by a masked rhs task)
struct Form { int nins; bool inv; int rd[8][2]; };
constexpr Form kFull = {8, false, {{3, 0}, {3, 16}, {1, 0}, {2, 0}, {2, 16}, {0, 0}, {1, 16}, {0, 16}}};
constexpr Form kHalf = {6, false, {{3, 0}, {3, 16}, {1, 0}, {2, 0}, {2, 16}, {0, 0}}};
constexpr Form kQuarter = {5, false, {{3, 0}, {3, 16}, {1, 0}, {2, 0}, {0, 0}}};
constexpr Form kInv = {3, true, {{0, 0}, {0, 16}, {1, 0}}};
constexpr Form kBwd = {6, false, {{1, 0}, {1, 16}, {2, 0}, {2, 16}, {3, 0}, {0, 0}}};
constexpr Form kBwdHalf = {5, false, {{1, 0}, {1, 16}, {2, 0}, {3, 0}, {0, 0}}};
// Modelled extra LDS cycles of one pass in form fm: operand(slot, ins, field) = the byte offset lane slot's descriptor holds for that read, or
// -1 if the lane takes no part in the instruction.  Operands that are written back (field 0 = T / y_i; D and y of an inversion) hit the same
// banks a second time with the slower store instruction: ww weighs their conflicts (SymOpts::place_ww in the placement search, 1 elsewhere).
template <class F>
long form_conflicts(const Form& fm, int rowl, int row_bytes, long ww, F&& operand)
{
    long cost = 0;
    for (int ins = 0; ins < fm.nins; ++ins) {
        BankCount bc;
        for (int lane = 0; lane < 64; ++lane) {
            const int o = operand(lane % rowl, ins, fm.rd[ins][0]);
            if (o >= 0) bc.add(lane, (lane / rowl) * row_bytes + o + fm.rd[ins][1]);
        }
        cost += bc.extra() * ((fm.inv || fm.rd[ins][0] == 0) ? ww : 1);
    }
    return cost;
}

// A pass in half / quarter form holds `lanes` lanes per task of the full form: what lane k adds to each descriptor field (offsets in doubles,
// relmc_dev.h).  rhs: field 0 may carry the rhs flag, and such a task has one row only, the first half of its lanes.
struct Expansion { int lanes; bool rhs; int add[4][4]; };
constexpr Expansion kHalfUpd = {2, true, {{0, 0, 0, 0}, {2, 2, 0, 0}}};                                       // lane r: (&T[r][0], &Wa[r][0], Wb, D)
constexpr Expansion kQuarterUpd = {4, true, {{0, 0, 0, 0}, {1, 0, 2, 0}, {2, 2, 0, 0}, {3, 2, 2, 0}}};         // lane 2r + c: (&T[r][c], &Wa[r][0], &Wb[c][0], D)
constexpr Expansion kHalfBwd = {2, false, {{0, 0, 0, 0}, {1, 0, 2, 0}}};                                       // lane r: (&Y_i[r], W, &P_i[r][0], Y_a)

struct Task { uint8_t kind; uint16_t o[4]; std::vector<int> rd, wr; };      // kind 0 update, 1 inversion, 2 back substitution; read / written units
enum class Pack { ok, no_fit, cycle };
constexpr int kNever = 1 << 30;              // pass index from which the half capacity applies: none

// What the steps of case_symbolic hand to each other (host only); every step is a member, case_symbolic alone knows their order.
template <class TL>
struct Symbolic {
    static constexpr int NBT = TL::NBT, NLT = TL::NLT, NIT = TL::NIT, NCOMPMAX = TL::NCOMPMAX, MAXOFF = TL::MAXOFF, MAXPASS = TL::MAXPASS,
                         ROWL = TL::RW, IS = TL::IS, WPB = TL::WPB, SPW = TL::SPW, OW = TL::OW;
    const relmc_case_desc* d; DevCaseT<TL>& C; const int order_variant; const SymOpts& so; SymGeom& geom; std::string& err;
    const int nb, ng, nl, nd, ninj, ncomp;
    std::vector<int> ext2int;                 // external bus -> internal bus = elimination step
    std::vector<std::vector<int>> N;          // higher neighbours, internal ids, ascending
    std::vector<std::vector<int>> blk;        // blk[a][i], a > i: id of the off-diagonal block, -1 = none
    std::vector<int> pos;                     // block id -> position in W (diagonal blocks stay at their bus index)
    int noff = 0;
    std::vector<Task> tasks;                  // in sequential (right-looking) order
    std::vector<std::vector<int>> strict, weak;      // per task: tasks that must be in an EARLIER pass / in an earlier or the SAME pass
    std::vector<int> depth;                   // longest remaining dependency path within the task's phase
    std::vector<int> pkind, pcount;           // per pass: kind, tasks
    std::vector<std::vector<int>> pass_tasks; // pass -> RW slots, task index or -1
    int nup = 0, first_bwd = 0;               // update passes; the first back-substitution pass
    int nfull_upd = 0, nhalf_end = 0;         // update passes [0, nfull_upd) are in full form, [nfull_upd, nhalf_end) in half form, the rest in quarter form
    uint32_t stride = 0, stash_off = 0;       // doubles between two scenario rows' workspaces in LDS; where a row's stash begins

    Symbolic(const relmc_case_desc* d_, DevCaseT<TL>& C_, int variant, const SymOpts& so_, SymGeom& geom_, std::string& err_)
        : d(d_), C(C_), order_variant(variant), so(so_), geom(geom_), err(err_), nb(d_->nb), ng(d_->ng), nl(d_->nl), nd(d_->nd), ninj(d_->ng + d_->nd), ncomp(d_->ng + d_->nl) {}
    int failx(int code, const char* msg) { err = msg; return code; }
    int offd(int i) const { return 4 * i; }
    int offb(int a, int i) const { return 4 * pos[blk[a][i]]; }
    int offy(int i) const { return (int)C.off_rhs + 2 * i; }
    int offp(int i) const { return 4 * i; }                          // P = inv(D) overwrites D in place
    int unit(int off) const { return off < (int)C.off_rhs ? off >> 2 : (int)C.off_rhs / 4 + ((off - (int)C.off_rhs) >> 1); }   // one block / one rhs pair
    int remap(int o) const                                           // offset under the identity placement -> current placement
    {
        const int f = o & 0x8000; o &= 0x7fff;
        if (o >= 4 * nb && o < (int)C.off_rhs) o = 4 * pos[o >> 2] + (o & 3);
        return o | f;
    }

    int header()
    {
        if (nb > NBT || nl > NLT || ninj > NIT || ncomp > NCOMPMAX || nl > 126 || ninj > 254)
            return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: case exceeds the compiled tiles (128 buses, 126 lines, 192 injections, 256 components)");
        std::memset(&C, 0, sizeof(C));
        C.nb = nb; C.ng = ng; C.nl = nl; C.nd = nd; C.ninj = ninj; C.ncomp = ncomp;
        C.base_mva = d->base_mva; C.total_load = d->total_load;
        C.exist_mask = nb >= 32 ? 0xffffffffu : ((1u << nb) - 1u);      // used by the 16-lane tile only (nb <= 32 there)
        return RELMC_OK;
    }
    // ---- elimination order on the bus graph (all lines in service = superset of every outage state): level-then-min-fill, reference bus last
    int elimination_order()
    {
        std::vector<std::vector<char>> A(nb, std::vector<char>(nb, 0));
        for (int l = 0; l < nl; ++l) {
            const int f = d->br_from[l], t = d->br_to[l];
            if (f < 0 || f >= nb || t < 0 || t >= nb || f == t || !(d->br_b[l] == d->br_b[l]))
                return failx(RELMC_ERR_INVALID, "relmc_case_load: bad branch end points");
            A[f][t] = A[t][f] = 1;
        }
        std::vector<int> level(nb, -1);
        std::vector<char> gone(nb, 0);
        std::vector<std::vector<int>> hi_ext(nb);          // higher neighbours (external ids) at elimination time
        ext2int.assign(nb, -1);
        // The primary order may come from the host (relmc_case_order_hint: an order tuned offline by relmc_tune_order against this very
        // scheduler); the further orders of the retry path stay rule-made.
        std::vector<int> forced;
        if (order_variant == 0 && so.order_hint && so.n_hint > 0) forced.assign(so.order_hint, so.order_hint + so.n_hint);
        if (!forced.empty()) {
            std::vector<char> seen(nb, 0);
            bool ok = (int)forced.size() == nb && forced.back() == d->ref_bus;
            for (int v : forced) { if (v < 0 || v >= nb || seen[v]) ok = false; else seen[v] = 1; }
            if (!ok) return failx(RELMC_ERR_INVALID, "relmc_case_load: the elimination-order hint is not a permutation of the buses with the reference bus last");
        }
        for (int step = 0; step < nb; ++step) {
            int best = -1; long bestkey = 0;
            if (!forced.empty()) best = forced[step];
            else
            for (int b = 0; b < nb; ++b) {
                if (gone[b] || (b == d->ref_bus && step < nb - 1)) continue;
                int deg = 0, fillc = 0, lev = 0;
                for (int x = 0; x < nb; ++x) {
                    if (x == b || !A[b][x]) continue;
                    if (gone[x]) { if (level[x] + 1 > lev) lev = level[x] + 1; continue; }
                    deg++;
                    for (int y = x + 1; y < nb; ++y) if (!gone[y] && y != b && A[b][y] && !A[x][y]) fillc++;
                }
                // shallow elimination tree first (fewer dependent passes), then little fill
                long key = ((long)lev * 1000 + fillc) * 10000 + deg * 100 + b;
                if (order_variant == 1) key = ((long)lev * 1000 + fillc) * 10000 + deg * 100 + (nb - 1 - b);       // other tie-breaks
                else if (order_variant == 2) key = ((long)fillc * 1000 + lev) * 10000 + deg * 100 + b;            // fill first

                if (best < 0 || key < bestkey) { best = b; bestkey = key; }
            }
            int lev = 0;
            for (int x = 0; x < nb; ++x) if (x != best && A[best][x] && gone[x] && level[x] + 1 > lev) lev = level[x] + 1;
            level[best] = lev;
            for (int x = 0; x < nb; ++x) if (!gone[x] && x != best && A[best][x]) {
                hi_ext[best].push_back(x);
                for (int y = 0; y < nb; ++y) if (!gone[y] && y != best && y != x && A[best][y]) A[x][y] = A[y][x] = 1;      // symbolic fill
            }
            gone[best] = 1;
            ext2int[best] = step;
        }
        for (int i = 0; i < NBT; ++i) { C.b_ext[i] = 0xff; C.b_int[i] = 0xff; C.b_vinj[i] = -1; }
        for (int e = 0; e < nb; ++e) { C.b_ext[ext2int[e]] = (uint8_t)e; C.b_int[e] = (uint8_t)ext2int[e]; }
        C.ref_bus = ext2int[d->ref_bus];                    // == nb - 1
        N.assign(nb, {});
        for (int e = 0; e < nb; ++e) {
            for (int x : hi_ext[e]) N[ext2int[e]].push_back(ext2int[x]);
            std::sort(N[ext2int[e]].begin(), N[ext2int[e]].end());
        }
        return RELMC_OK;
    }
    // ---- block storage: diagonal blocks, off-diagonal blocks (a, i) a > i, rhs blocks, P blocks; the per-scenario LDS stride that follows from it
    int block_layout()
    {
        blk.assign(nb, std::vector<int>(nb, -1));
        for (int i = 0; i < nb; ++i) for (int a : N[i]) blk[a][i] = nb + noff++;
        if (noff > MAXOFF) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: too much fill for the solver workspace");
        C.noff = noff;
        C.off_rhs = (uint16_t)(4 * (nb + noff));          // rhs / solution: 2 doubles per bus
        C.off_p = 0;                                        // P = inv(D) overwrites D in place
        C.nws = (uint32_t)C.off_rhs + 2u * nb;
        if (C.nws >= 0x1000u) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: solver workspace too large");      // byte offsets of the pass descriptors keep bit 15 free
        pos.resize(nb + noff);
        for (int k = 0; k < nb + noff; ++k) pos[k] = k;
        scenario_stride();
        return RELMC_OK;
    }
    // doubles between two scenario rows' workspaces in LDS: what the placement model, the shadow rewrite and the launch geometry all go by
    void scenario_stride()
    {
        const uint32_t eval_doubles = 4u * (nl + 1) + 4u * (ninj + 1);   // line / injection records (+1 zero record each): alias the workspace
        uint32_t scen = C.nws > eval_doubles ? C.nws : eval_doubles;
        scen = (scen + 1u) & ~1u;
        stash_off = scen;
        scen += 2u * IS * ROWL + 2u + NBT + OW / 2u;           // stash: 1/D and Np/D per injection lane (+ one zero pair); lambda per bus; outage mask words
        while ((scen & 3u) != 2u) scen += 1;                  // 16-byte aligned rows (ds_read_b128!) whose 16-B slot index differs by an odd number
        scen += 4u * (uint32_t)so.scen_pad4;                   // (ablation builds: more padding between the rows, in steps of 32 bytes)
        stride = scen;
    }
    // ---- task list in sequential (right-looking) order
    int task_list()
    {
        // model only (SymOpts::model_leaf_free, with RELMC_VERBOSE): what would the update phase look like if the pivots that are complete at
        // assembly (no earlier-eliminated neighbour) were eliminated by the assembling lanes?  The printed schedule is NOT a valid program.
        std::vector<char> leaf_free(nb, 0);
        if (so.model_leaf_free >= 0) {
            const int maxdeg_free = so.model_leaf_free;
            std::vector<char> has_lower(nb, 0);
            for (int i = 0; i < nb; ++i) for (int a2 : N[i]) has_lower[a2] = 1;
            int nfree = 0, ntask_free = 0;
            for (int i = 0; i < nb; ++i) if (!has_lower[i] && (int)N[i].size() <= maxdeg_free) { leaf_free[i] = 1; nfree++; ntask_free += (int)(N[i].size() * (N[i].size() + 1) / 2 + N[i].size()); }
            fprintf(stderr, "relmc: model: %d pivots complete at assembly with <= %d higher neighbours, %d update tasks\n", nfree, maxdeg_free, ntask_free);
        }
        auto add = [&](int kind, int o0, int o1, int o2, int o3, std::vector<int> rd, std::vector<int> wr) {
            Task t; t.kind = (uint8_t)kind; t.o[0] = (uint16_t)o0; t.o[1] = (uint16_t)o1; t.o[2] = (uint16_t)o2; t.o[3] = (uint16_t)o3;
            t.rd = std::move(rd); t.wr = std::move(wr);
            tasks.push_back(std::move(t));
        };
        for (int i = 0; i < nb; ++i) {
            if (leaf_free[i]) continue;
            for (size_t ia = 0; ia < N[i].size(); ++ia)
                for (size_t ib = 0; ib <= ia; ++ib) {
                    const int a2 = N[i][ia], b2 = N[i][ib];
                    if (a2 != b2 && blk[a2][b2] < 0) return failx(RELMC_ERR_INVALID, "relmc_case_load: symbolic factorisation inconsistent");
                    const int T = a2 == b2 ? offd(a2) : offb(a2, b2);
                    add(0, T, offb(a2, i), offb(b2, i), offd(i), {unit(offb(a2, i)), unit(offb(b2, i)), unit(offd(i)), unit(T)}, {unit(T)});
                }
            for (int a2 : N[i])                               // right-hand side as a pseudo-bus: y_a' -= y_i' P W_a'
                add(0, offy(a2) | 0x8000, offy(i), offb(a2, i), offd(i), {unit(offy(i)), unit(offb(a2, i)), unit(offd(i)), unit(offy(a2))}, {unit(offy(a2))});
        }
        for (int i = 0; i < nb; ++i) add(1, offd(i), offy(i), 0, 0, {unit(offd(i)), unit(offy(i))}, {unit(offd(i)), unit(offy(i))});
        for (int a2 = nb - 1; a2 >= 0; --a2)
            for (int i = 0; i < a2; ++i)
                if (blk[a2][i] >= 0) add(2, offy(i), offb(a2, i), offp(i), offy(a2), {unit(offp(i)), unit(offb(a2, i)), unit(offy(a2)), unit(offy(i))}, {unit(offy(i))});
        return RELMC_OK;
    }
    // ---- dependencies in the sequential order of `tasks`: read-after-write and write-after-write need a LATER pass (strict), write-after-read
    // allows the SAME pass (weak: all lanes load before any lane stores); depth = longest remaining path within the phase
    void dependencies()
    {
        const int nt = (int)tasks.size(), nunits = (int)C.nws / 2 + 2;
        strict.assign(nt, {}); weak.assign(nt, {});
        std::vector<std::vector<int>> succ(nt);
        std::vector<std::vector<char>> succw(nt);                       // parallel to succ: 1 = strict edge
        std::vector<int> lw(nunits, -1);
        std::vector<std::vector<int>> readers(nunits);
        for (int i = 0; i < nt; ++i) {
            const Task& t = tasks[i];
            for (int r : t.rd) if (lw[r] >= 0) strict[i].push_back(lw[r]);
            for (int w : t.wr) {
                if (lw[w] >= 0) strict[i].push_back(lw[w]);
                for (int q : readers[w]) if (q != i) weak[i].push_back(q);
            }
            for (int r : t.rd) readers[r].push_back(i);
            for (int w : t.wr) { lw[w] = i; readers[w].clear(); }
        }
        for (int i = 0; i < nt; ++i) {
            for (int q : strict[i]) { succ[q].push_back(i); succw[q].push_back(1); }
            for (int q : weak[i]) { succ[q].push_back(i); succw[q].push_back(0); }
        }
        depth.assign(nt, 0);
        for (int i = nt - 1; i >= 0; --i)
            for (size_t k = 0; k < succ[i].size(); ++k) {
                const int j = succ[i][k];
                if (tasks[j].kind == tasks[i].kind && depth[j] + succw[i][k] > depth[i]) depth[i] = depth[j] + succw[i][k];
            }
        if (verbose()) {         // longest dependency chain per phase = the fewest passes any packing could reach
            int md[3] = {0, 0, 0};
            for (int i = 0; i < nt; ++i) if (depth[i] + 1 > md[tasks[i].kind]) md[tasks[i].kind] = depth[i] + 1;
            fprintf(stderr, "relmc: order %d: critical path (passes) update %d, inversion %d, back substitution %d\n", order_variant, md[0], md[1], md[2]);
        }
    }
    // List scheduling by longest remaining dependency path (round 2; the round-1 scheduler placed the tasks as soon as possible in
    // generation order and needed one more update pass on both test systems): packs the tasks of one kind into passes appended to `passes`
    // (pass index = position there), RW tasks per pass, RW / 2 in update passes from pass half_from on.
    Pack pack(int kind, int half_from, std::vector<int>& passof, std::vector<std::vector<int>>& passes) const
    {
        const int nt = (int)tasks.size();
        std::vector<int> remaining, ready, rest;
        std::vector<char> in_pass(nt);
        for (int i = 0; i < nt; ++i) if (tasks[i].kind == kind) remaining.push_back(i);
        while (!remaining.empty()) {
            const int cur = (int)passes.size();
            if (cur >= MAXPASS - 1) return Pack::no_fit;
            ready.clear();
            for (int i : remaining) {
                bool ok = true;
                for (int q : strict[i]) if (passof[q] < 0 || passof[q] >= cur) { ok = false; break; }
                if (ok) ready.push_back(i);
            }
            std::stable_sort(ready.begin(), ready.end(), [&](int a2, int b2) { return depth[a2] != depth[b2] ? depth[a2] > depth[b2] : a2 < b2; });
            const int cap = (kind == 0 && cur >= half_from) ? ROWL / 2 : ROWL;
            std::vector<int> chosen;
            std::fill(in_pass.begin(), in_pass.end(), 0);
            for (int i : ready) {
                if ((int)chosen.size() >= cap) break;
                bool ok = true;                                   // readers of what this task overwrites: already placed, or in this pass
                for (int q : weak[i]) if (passof[q] < 0 && !in_pass[q]) { ok = false; break; }
                if (ok) { chosen.push_back(i); in_pass[i] = 1; }
            }
            if (chosen.empty()) return Pack::cycle;
            for (int i : chosen) passof[i] = cur;
            passes.push_back(std::move(chosen));
            rest.clear();
            for (int i : remaining) if (passof[i] < 0) rest.push_back(i);
            remaining.swap(rest);
        }
        return Pack::ok;
    }
    // ---- scheduling.  Phases stay contiguous: all PK_UPD passes, then PK_INV, then PK_BWD.
    int schedule()
    {
        for (int q = 0; q < MAXPASS; ++q) for (int r = 0; r < ROWL; ++r) for (int k = 0; k < 4; ++k) C.task[q][r][k] = 0xffff;   // null task
        std::vector<int> passof(tasks.size(), -1);
        // A pass costs its LDS instructions whatever its fill, and an update pass filled to at most a half / a quarter runs in the
        // cheaper half / quarter form (relmc_dev.h): 10 / 7 / 6 instructions.  So the update phase is scheduled twice or more: with
        // the full row width throughout, and with only half of it from pass F on; the cheapest variant that needs no extra pass wins.
        int best_f = kNever;
        long best_cost = -1; size_t best_n = 0;
        for (int trial = -1; trial < MAXPASS; ++trial) {
            std::vector<int> po(passof);
            std::vector<std::vector<int>> tp;
            if (pack(0, trial < 0 ? kNever : trial, po, tp) != Pack::ok) { if (trial < 0) break; else continue; }      // this trial does not count
            long c = 0;
            for (const auto& p : tp) c += (int)p.size() > ROWL / 2 ? 10 : ((int)p.size() > ROWL / 4 ? 7 : 6);
            if (trial < 0) { best_cost = c; best_n = tp.size(); }
            else if (tp.size() <= best_n && c < best_cost) { best_cost = c; best_f = trial; }
            if (trial >= 0 && (size_t)trial >= best_n) break;
        }
        if (so.no_quarter) best_f = kNever;
        std::vector<std::vector<int>> passes;
        for (int kind = 0; kind < 3; ++kind) {
            const Pack r = pack(kind, best_f, passof, passes);
            if (r == Pack::no_fit) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: solver schedule exceeds MAXPASS");
            if (r == Pack::cycle) return failx(RELMC_ERR_INVALID, "relmc_case_load: solver schedule has a dependency cycle");
            pkind.resize(passes.size(), kind);
        }
        for (const auto& p : passes) {
            pcount.push_back((int)p.size()); pass_tasks.push_back(std::vector<int>(ROWL, -1));
            std::copy(p.begin(), p.end(), pass_tasks.back().begin());
        }
        const int np = (int)pkind.size();
        for (int q = 0; q < np; ++q) if (pkind[q] == 0) nup++;
        while (first_bwd < np && pkind[first_bwd] != 2) first_bwd++;
        return RELMC_OK;
    }
    // modelled extra LDS cycles of pass p's operand reads on the task list under the current placement (full forms: the forms come later)
    long pass_cost(int p) const
    {
        const int kind = pkind[p];
        const std::vector<int>& pt = pass_tasks[p];
        return form_conflicts(kind == 0 ? kFull : (kind == 1 ? kInv : kBwd), ROWL, 8 * (int)stride, so.place_ww, [&](int slot, int ins, int f) {
            if (pt[slot] < 0) return -1;
            const Task& t = tasks[pt[slot]];
            if (kind == 0 && ins >= 6 && (t.o[0] & 0x8000)) return -1;                // rhs-row tasks skip the second halves of T and Wa
            return 8 * (remap(t.o[f]) & 0x7fff);
        });
    }
    // ---- LDS bank-conflict aware placement (host only; the passes and their dependencies are untouched).  Two degrees of freedom cost
    // nothing at run time: where the off-diagonal blocks live in W and which lane of the row carries which task of a pass.  A seeded
    // local search minimises the modelled extra LDS cycles of all operand reads of one Newton step.
    void place()
    {
        const int np = (int)pkind.size();
        std::vector<long> pc(np);
        long total = 0;
        for (int p = 0; p < np; ++p) { pc[p] = pass_cost(p); total += pc[p]; }
        const long before = total;
        uint64_t rng = 0x9E3779B97F4A7C15ull;
        auto rnd = [&](int m) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (int)((rng >> 33) % (uint64_t)m); };
        std::vector<std::vector<int>> passes_of_block(nb + noff);      // passes whose operands include the block
        for (int p = 0; p < np; ++p)
            for (int r = 0; r < ROWL; ++r) {
                const int ti = pass_tasks[p][r];
                if (ti < 0) continue;
                for (int k = 0; k < 4; ++k) {
                    const int o = tasks[ti].o[k] & 0x7fff;
                    if (o >= 4 * nb && o < (int)C.off_rhs && !(tasks[ti].kind == 1 && k >= 2)) {
                        std::vector<int>& v = passes_of_block[o >> 2];
                        if (std::find(v.begin(), v.end(), p) == v.end()) v.push_back(p);
                    }
                }
            }
        std::vector<int> touched; std::vector<long> newc;
        // 100 moves per block: 36 / 114 ms of relmc_case_load on RTS-24 / RTS-96; 400 (round 1) took 144 / 440 ms for kernel times within
        // run-to-run noise of these (19.0 vs 19.2 ms, 78.4 vs 78.2 ms per 1e6); no search at all: 19.2 / 79.3 ms
        const int moves = noff > 0 ? so.place_moves * (nb + noff) : 0;
        for (int it = 0; it < moves && total > 0; ++it) {
            if (rnd(10) < 6) {                                  // swap the positions of two off-diagonal blocks
                const int i = nb + rnd(noff), j = nb + rnd(noff);
                if (i == j) continue;
                std::swap(pos[i], pos[j]);
                touched.clear();
                for (int p : passes_of_block[i]) touched.push_back(p);
                for (int p : passes_of_block[j]) if (std::find(touched.begin(), touched.end(), p) == touched.end()) touched.push_back(p);
                long delta = 0; newc.resize(touched.size());
                for (size_t k = 0; k < touched.size(); ++k) { newc[k] = pass_cost(touched[k]); delta += newc[k] - pc[touched[k]]; }
                if (delta <= 0) { total += delta; for (size_t k = 0; k < touched.size(); ++k) pc[touched[k]] = newc[k]; }
                else std::swap(pos[i], pos[j]);
            } else {                                            // swap two lanes (tasks or holes) of one pass
                const int p = rnd(np), i = rnd(ROWL), j = rnd(ROWL);
                if (i == j) continue;
                std::swap(pass_tasks[p][i], pass_tasks[p][j]);
                const long c2 = pass_cost(p);
                if (c2 <= pc[p]) { total += c2 - pc[p]; pc[p] = c2; } else std::swap(pass_tasks[p][i], pass_tasks[p][j]);
            }
        }
        geom.conflict_before = before; geom.conflict_after = total;
        for (int p = 0; p < np; ++p)
            for (int r = 0; r < ROWL; ++r) {
                const int ti = pass_tasks[p][r];
                if (ti < 0) continue;
                for (int k = 0; k < 4; ++k) C.task[p][r][k] = (uint16_t)remap(tasks[ti].o[k]);
                if (tasks[ti].kind == 1) { C.task[p][r][2] = 0; C.task[p][r][3] = 0; }
            }
    }
    // compacts the tasks of pass p and re-emits each on ex.lanes consecutive lanes
    void expand(int p, const Expansion& ex)
    {
        uint16_t full[ROWL][4]; int nfull = 0;
        for (int r = 0; r < ROWL; ++r) if (C.task[p][r][0] != 0xffff) { for (int k = 0; k < 4; ++k) full[nfull][k] = C.task[p][r][k]; nfull++; }
        for (int r = 0; r < ROWL; ++r) for (int k = 0; k < 4; ++k) C.task[p][r][k] = 0xffff;
        for (int t = 0; t < nfull; ++t) {
            const bool vec = ex.rhs && (full[t][0] & 0x8000u) != 0;
            if (ex.rhs) full[t][0] &= 0x7fff;
            for (int k = 0; k < (vec ? ex.lanes / 2 : ex.lanes); ++k)
                for (int f = 0; f < 4; ++f) C.task[p][ex.lanes * t + k][f] = (uint16_t)(full[t][f] + ex.add[k][f]);
        }
    }
    // ---- pass forms (relmc_dev.h): the sparsely filled PK_UPD passes at the end of the phase in quarter form, those in front of them in half
    // form; back-substitution passes filled to at most a half in half form (one LDS instruction less per pass)
    void pass_forms()
    {
        int nq = 0;
        while (nq < nup && pcount[nup - 1 - nq] <= ROWL / 4 && !so.no_quarter) nq++;
        C.npass_updq = (uint16_t)nq;
        int nh = 0;
        while (nq + nh < nup && pcount[nup - 1 - nq - nh] <= ROWL / 2 && !so.no_half && !so.no_quarter) nh++;
        C.npass_updh = (uint16_t)nh;
        nfull_upd = nup - nq - nh; nhalf_end = nup - nq;
        for (int p = nfull_upd; p < nhalf_end; ++p) expand(p, kHalfUpd);
        for (int p = nhalf_end; p < nup; ++p) expand(p, kQuarterUpd);
        C.bwd_half = 0;
        if (so.no_bwd_half) return;
        const int np = (int)pkind.size();
        // all or nothing: a loop that switches form per pass costs more than the half form saves (measured: +1.6 % / +2.5 % against the
        // full form alone, profiles/r3_pf/c26_notes.txt), so the half form is taken when EVERY pass qualifies (RTS-96: 11 of 11; RTS-24: 5 of 7, stays full)
        // The 16-lane tile keeps the full form: its kernel is 0.35 % slower with the second loop compiled in, whatever runs.
        bool all_half = ROWL == 64 && np - first_bwd <= 64 && first_bwd < np;
        for (int p = first_bwd; p < np; ++p) if (pcount[p] > ROWL / 2) all_half = false;
        for (int p = first_bwd; all_half && p < np; ++p) { expand(p, kHalfBwd); C.bwd_half |= 1ull << (p - first_bwd); }
    }
    // The kernel adds a descriptor field to the workspace's LDS address as it is (one VALU instruction per operand instead of two): the
    // table holds BYTE offsets (< 32 KiB: a scenario's workspace is a fraction of the 160 KiB of LDS), bit 15 of field 0 = rhs task as before.
    void byte_offsets()
    {
        for (size_t q = 0; q < pkind.size(); ++q)
            for (int r = 0; r < ROWL; ++r) {
                if (C.task[q][r][0] == 0xffff) continue;
                for (int k = 0; k < 4; ++k) {
                    const uint32_t v = C.task[q][r][k], f = (k == 0 && (int)q < nfull_upd) ? (v & 0x8000u) : 0u;      // only the full-form update passes carry the rhs flag
                    C.task[q][r][k] = (uint16_t)(((v & (f ? 0x7fffu : 0xffffu)) << 3) | f);
                }
            }
    }

    const Form& form_of(int p) const
    {
        if (pkind[p] == 0) return p < nfull_upd ? kFull : (p < nhalf_end ? kHalf : kQuarter);
        if (pkind[p] == 1) return kInv;
        return ((C.bwd_half >> (p - first_bwd)) & 1) ? kBwdHalf : kBwd;
    }
    // modelled extra LDS cycles of the pass's operand reads on the byte-offset image: lanes with field 0 = 0xffff take no part;
    // mode 0 = the masked kernel (idle lanes and an rhs task's second row off), 1 = the tasks alone with both rows read by every one of
    // them (what the shadowing kernel's active lanes do), 2 = the shadowing kernel (every lane reads everything)
    long image_cost(int p, int mode) const
    {
        const bool all = mode == 2, inv = pkind[p] == 1, full = pkind[p] == 0 && p < nfull_upd;
        return form_conflicts(form_of(p), ROWL, 8 * (int)stride, 1, [&](int slot, int ins, int f) {
            const uint16_t* t = C.task[p][slot];
            if (t[0] == 0xffff && t[3] == 0xffff) return -1;                 // not assigned yet
            if (!all && (task_idle(t, inv) || (mode == 0 && full && ins >= 6 && (t[0] & 0x8000u)))) return -1;
            return (int)((f == 0 && full) ? (t[0] & 0x7fffu) : t[f]);
        });
    }
    // Idle lanes shadow an active lane (relmc_dev.h, "idle lanes"): the last rewrite of the finished pass program.  Every lane without a
    // task gets the read operands of an active lane of its pass plus the form's idle marker, so the kernel may run a pass's loads and
    // arithmetic on all 64 lanes and predicate only the stores.  Equal addresses are broadcasts to the LDS, so a shadow inside the same
    // b128 read group adds no bank conflict to the operands it copies; the one field the marker occupies (T / Y_i := the pivot field) is a
    // new address in that operand's read.  The shadowed lane is therefore chosen per pass and read group by the placement model itself:
    // the active lane OF THE SAME READ GROUP that leaves the pass's modelled conflicts lowest (ties: the lowest lane; any lane of the pass where the
    // group holds no task: its lanes then read one address all together).  A pass always holds a task: the scheduler refuses an empty one above.
    int shadow_idle_lanes()
    {
        const int np = (int)pkind.size();
        long masked = 0, tasks_all_rows = 0, shadowed = 0;
        const bool model = so.place_moves > 0;               // the order tuner evaluates thousands of orders without placing them: first candidate, no model
        for (int p = 0; p < np; ++p) {
            const bool inv = pkind[p] == 1;
            std::vector<int> active;
            for (int r = 0; r < ROWL; ++r) {
                const uint16_t* t = C.task[p][r];
                if (t[0] == 0xffff) continue;
                // no real task carries the idle marker: an update's target is an off-diagonal block, a LATER bus' diagonal block or an rhs pair,
                // never its own pivot; a back substitution's y_i and y_a belong to different buses; an inversion's last two fields are zero
                if (task_idle(t, inv)) return failx(RELMC_ERR_INVALID, "relmc_case_load: a solver task carries the idle marker");
                active.push_back(r);
            }
            if (active.empty()) return failx(RELMC_ERR_INVALID, "relmc_case_load: a solver pass without a task");
            if (model) { masked += image_cost(p, 0); tasks_all_rows += image_cost(p, 1); }
            const int ngroup = ROWL == 64 ? 4 : 2;                                       // lanes that share their b128 read groups in every scenario row
            for (int g = 0; g < ngroup; ++g) {
                std::vector<int> idle;
                for (int r = 0; r < ROWL; ++r) if (C.task[p][r][0] == 0xffff && kGroupOfLane[r] == g) idle.push_back(r);
                if (idle.empty()) continue;
                std::vector<int> cand;
                for (int r : active) if (kGroupOfLane[r] == g) cand.push_back(r);
                if (cand.empty()) cand = active;                  // no task among these lanes: any lane of the pass (they all read one address then)
                auto assign = [&](int src) {
                    for (int r : idle) {
                        uint16_t* q = C.task[p][r]; const uint16_t* s = C.task[p][src];
                        if (inv) { q[0] = s[0]; q[1] = s[1]; q[2] = TASK_IDLE_INV; q[3] = TASK_IDLE_INV; }
                        else { q[0] = s[3]; q[1] = s[1]; q[2] = s[2]; q[3] = s[3]; }
                    }
                };
                int best = -1; long bestc = 0;
                for (int src : cand) { if (!model) { best = src; break; } assign(src); const long c = image_cost(p, 2); if (best < 0 || c < bestc) { best = src; bestc = c; } }
                assign(best);
            }
            if (model) shadowed += image_cost(p, 2);
        }
        geom.shadow_masked = masked; geom.shadow_tasks = tasks_all_rows; geom.shadow_all = shadowed;
        if (verbose()) fprintf(stderr, "relmc: order %d: modelled LDS conflict cycles of the device image, idle lanes masked %ld, the tasks with every second row read %ld, idle lanes shadowing %ld\n", order_variant, masked, tasks_all_rows, shadowed);
        return RELMC_OK;
    }

    int pass_counts()
    {
        const int np = (int)pkind.size();
        C.npass = (uint16_t)np;
        for (int q = 0; q < np; ++q) {
            C.pass_ntask[q] = (uint8_t)pcount[q];
            // kinds must appear as contiguous phases UPD.. INV.. BWD..
            if (q > 0 && pkind[q] < pkind[q - 1]) return failx(RELMC_ERR_INVALID, "relmc_case_load: schedule phases out of order");
        }
        C.npass_upd = (uint16_t)nup; C.npass_inv = (uint16_t)(first_bwd - nup);
        if (verbose()) { fprintf(stderr, "relmc: order %d: %d + %d + %d passes, tasks per pass:", order_variant, nup, first_bwd - nup, np - first_bwd); for (int q = 0; q < np; ++q) fprintf(stderr, " %d", pcount[q]); fprintf(stderr, "\n"); }
        return RELMC_OK;
    }
    // ---- lines
    int lines()
    {
        for (int l = 0; l < NLT; ++l) C.l_partner[l] = -1;
        std::vector<int> pair_owner((size_t)nb * nb, -1), pair_lines((size_t)nb * nb, 0);
        std::vector<char> has_line(nb + noff, 0);
        for (int l = 0; l < nl; ++l) {
            const int f = ext2int[d->br_from[l]], t = ext2int[d->br_to[l]];
            const int lo = f < t ? f : t, hi = f < t ? t : f;
            uint32_t flags = LF_EXISTS;
            if (d->br_rate[l] != 0.0) flags |= LF_LIMITED;
            const size_t key = (size_t)hi * nb + lo;
            if (pair_owner[key] < 0) {
                pair_owner[key] = l; flags |= LF_OWNER;
                if (blk[hi][lo] < 0) return failx(RELMC_ERR_INVALID, "relmc_case_load: line outside the symbolic pattern");
                C.l_blk[l] = (uint16_t)offb(hi, lo);
                has_line[blk[hi][lo]] = 1;
            } else {
                if (pair_lines[key] >= 2) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: more than two parallel lines");
                C.l_partner[pair_owner[key]] = l;
            }
            pair_lines[key]++;
            C.l_b[l] = d->br_b[l];
            C.l_rate[l] = d->br_rate[l] / d->base_mva;
            C.l_info[l] = (uint32_t)f | ((uint32_t)t << 8) | (flags << 24);
            for (int side = 0; side < 2; ++side) {
                const int bus = side ? t : f;
                if (C.b_nline[bus] >= DEGMAX) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: more than 8 lines at a bus");
                C.b_line[bus][C.b_nline[bus]++] = (uint8_t)(l | (side ? 0x80 : 0));
            }
        }
        for (int i = 0; i < nb; ++i) {
            double s_ = 0.0; for (int e = 0; e < C.b_nline[i]; ++e) s_ += C.l_b[C.b_line[i][e] & 0x7f]; C.b_bsum[i] = s_;   // same order as the kernel's loop
            uint64_t pk = 0;
            for (int e = 0; e < 8; ++e) pk |= (uint64_t)(e < C.b_nline[i] ? C.b_line[i][e] : nl) << (8 * e);
            C.b_line8[i] = pk;
        }
        int nzero = 0;
        for (int k = nb; k < nb + noff; ++k) if (!has_line[k]) C.zero_off[nzero++] = (uint16_t)(4 * pos[k]);
        C.nzero = (uint16_t)nzero;
        return RELMC_OK;
    }
    // ---- injections
    int injections()
    {
        for (int j = 0; j < ninj; ++j) {
            if (d->inj_bus[j] < 0 || d->inj_bus[j] >= nb) return failx(RELMC_ERR_INVALID, "relmc_case_load: bad injection bus");
            const int bus = ext2int[d->inj_bus[j]];
            C.i_tab[j][0] = d->inj_pmax[j] / d->base_mva;
            C.i_tab[j][1] = d->inj_pmin[j] / d->base_mva;
            C.i_tab[j][2] = d->inj_cost[j] * d->base_mva;
            C.i_tab[j][3] = d->inj_pmin[j];
            C.i_info[j] = (uint32_t)bus | ((j < ng ? IK_REAL : IK_VIRTUAL) << 8);
            if (C.b_ninj[bus] >= BINJMAX) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: more than 8 injections at a bus");
            C.b_inj[bus][C.b_ninj[bus]++] = (uint8_t)j;
            if (j >= ng) {
                if (C.b_vinj[bus] >= 0) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: two virtual generators at one bus");
                C.b_vinj[bus] = (int16_t)j;
            }
        }
        int maxdeg = 0, maxinj = 0;
        for (int i = 0; i < nb; ++i) {
            uint64_t pk = 0;
            for (int e = 0; e < 8; ++e) pk |= (uint64_t)(e < C.b_ninj[i] ? C.b_inj[i][e] : ninj) << (8 * e);
            C.b_inj8[i] = pk;
            if (C.b_nline[i] > maxdeg) maxdeg = C.b_nline[i];
            if (C.b_ninj[i] > maxinj) maxinj = C.b_ninj[i];
        }
        C.maxdeg = (uint16_t)maxdeg; C.maxinj = (uint16_t)maxinj;
        return RELMC_OK;
    }
    // ---- which lane of which bus slot holds which bus in the vector phases.  A slot's gather loops run to the longest line / injection
    // list among its buses (two entries per step), so the partly filled second slot is given the buses with the shortest lists: the pair of
    // list-length limits (a, b) with the fewest steps that still admits nb - RW buses.  Everything is indexed by bus, so this is free.
    void bus_lanes()
    {
        for (int q = 0; q < NBT; ++q) C.b_lane[q] = 0xff;
        std::vector<int> slot_of(nb, 0);
        const int n1 = nb > ROWL ? nb - ROWL : 0;
        if (n1 > 0 && TL::BS == 2 && !so.no_bus_map) {
            int best_a = DEGMAX, best_b = BINJMAX, best_steps = 1 << 30;
            for (int a2 = 0; a2 <= DEGMAX; ++a2) for (int b2 = 0; b2 <= BINJMAX; ++b2) {
                int cnt = 0;
                for (int i = 0; i < nb; ++i) if (C.b_nline[i] <= a2 && C.b_ninj[i] <= b2) cnt++;
                const int steps = (a2 + 1) / 2 + (b2 + 1) / 2;
                if (cnt >= n1 && steps < best_steps) { best_steps = steps; best_a = a2; best_b = b2; }
            }
            std::vector<int> cand;
            for (int i = 0; i < nb; ++i) if (C.b_nline[i] <= best_a && C.b_ninj[i] <= best_b) cand.push_back(i);
            std::stable_sort(cand.begin(), cand.end(), [&](int x, int y) { return C.b_nline[x] + C.b_ninj[x] < C.b_nline[y] + C.b_ninj[y]; });
            for (int k = 0; k < n1; ++k) slot_of[cand[k]] = 1;
        } else {
            for (int i = 0; i < nb; ++i) slot_of[i] = i / ROWL;
        }
        int fill[TL::BS] = {};
        for (int i = 0; i < nb; ++i) {
            const int t = slot_of[i];
            C.b_lane[ROWL * t + fill[t]++] = (uint8_t)i;
            if (C.b_nline[i] > C.maxdeg_s[t]) C.maxdeg_s[t] = C.b_nline[i];
            if (C.b_ninj[i] > C.maxinj_s[t]) C.maxinj_s[t] = C.b_ninj[i];
        }
    }

    // ---- the fill-only blocks handed to the spare lanes of the assembly's block stores (relmc_dev.h: l_blk_fill, b_lane_fill).  Spare are the
    // lanes of the line slots without an owner line (slots behind nl, partner lines) and the lanes of the bus slots without a bus.  With more
    // fill blocks than spare lanes the first entries of zero_off, [0, nzero_res), keep the clearing loop.  l_blk, b_lane, zero_off and nzero stay.
    // Which lane takes which block is chosen by the modelled cost of the stores: a slot's lanes issue two 16-byte stores each (the block's
    // two halves), served in groups of 8 contiguous lanes with bank = (byte address / 4) mod 32 (MI355X_MICROARCH.md), so every different
    // 16-byte unit on one of a group's eight 4-bank sets is one LDS-array cycle, and a store costs the array cycles of all its groups or the
    // 13 cycles its operands take to reach the LDS, whichever is more.  The scenario rows of a wavefront add the same cycles each (their
    // workspaces differ by a common shift).  First fit, then exchanges of two lanes' targets while the modelled sum falls; the order tuner
    // (place_moves = 0: its cost does not read these tables) stops at first fit.
    long fill_slot_cost(const uint16_t* off) const      // off[ROWL]: W offset in doubles of the block a slot's lane stores, 0xffff = none
    {
        long cyc = 0;
        for (int g = 0; g < ROWL / 8; ++g) {
            int n[8] = {}, mx = 0; uint16_t seen[8][8];
            for (int r = 8 * g; r < 8 * g + 8; ++r) {
                if (off[r] == 0xffff) continue;
                const int set = (off[r] / 2) & 7;
                bool dup = false; for (int k = 0; k < n[set]; ++k) dup = dup || seen[set][k] == off[r];
                if (!dup) seen[set][n[set]++] = off[r];
                if (n[set] > mx) mx = n[set];
            }
            cyc += mx;
        }
        cyc *= SPW;
        return 2 * (cyc > 13 ? cyc : 13);
    }
    int fill_lanes()
    {
        for (int l = 0; l < NLT; ++l) C.l_blk_fill[l] = ((C.l_info[l] >> 24) & LF_OWNER) ? C.l_blk[l] : (uint16_t)0xffff;
        std::vector<uint16_t> boff(NBT);                 // the bus slots' targets as W offsets: 4 * position
        for (int q = 0; q < NBT; ++q) boff[q] = C.b_lane[q] == 0xff ? (uint16_t)0xffff : (uint16_t)(4 * C.b_lane[q]);
        std::vector<uint16_t*> spare;
        for (int l = 0; l < NLT; ++l) if (C.l_blk_fill[l] == 0xffff) spare.push_back(&C.l_blk_fill[l]);
        const int nspare_line = (int)spare.size();
        for (int q = 0; q < NBT; ++q) if (boff[q] == 0xffff) spare.push_back(&boff[q]);
        const int nres = C.nzero > spare.size() ? C.nzero - (int)spare.size() : 0;
        // a bus-slot lane tells a bus from a fill block by the position: diagonal blocks come first in W (relmc_dev.h)
        for (int z = nres; z < C.nzero; ++z) if (C.zero_off[z] < 4 * nb || C.zero_off[z] % 4) return failx(RELMC_ERR_INVALID, "relmc_case_load: fill block among the diagonal blocks");
        auto slot_of = [&](const uint16_t* t) { return t >= boff.data() && t < boff.data() + NBT ? boff.data() + (t - boff.data()) / ROWL * ROWL : C.l_blk_fill + (t - C.l_blk_fill) / ROWL * ROWL; };
        for (int z = nres, k = 0; z < C.nzero; ++z, ++k) *spare[k] = C.zero_off[z];
        for (int sweep = 0; sweep < 8 && so.place_moves > 0; ++sweep) {
            bool better = false;
            for (size_t i = 0; i < spare.size(); ++i) for (size_t j = i + 1; j < spare.size(); ++j) {
                if (*spare[i] == *spare[j]) continue;
                const uint16_t* si = slot_of(spare[i]); const uint16_t* sj = slot_of(spare[j]);
                const long before = fill_slot_cost(si) + (sj != si ? fill_slot_cost(sj) : 0);
                std::swap(*spare[i], *spare[j]);
                const long after = fill_slot_cost(si) + (sj != si ? fill_slot_cost(sj) : 0);
                if (after < before) better = true; else std::swap(*spare[i], *spare[j]);
            }
            if (!better) break;
        }
        int nline = 0, nbus = 0;
        for (int k = 0; k < (int)spare.size(); ++k) if (*spare[k] != 0xffff) { if (k < nspare_line) nline++; else nbus++; }
        for (int q = 0; q < NBT; ++q) C.b_lane_fill[q] = boff[q] == 0xffff ? (uint16_t)0xffff : (uint16_t)(boff[q] / 4);
        C.nfill_line = (uint16_t)nline; C.nfill_bus = (uint16_t)nbus; C.nzero_res = (uint16_t)nres;
        C.nidle_line = 0; C.nidle_bus_s[0] = C.nidle_bus_s[1] = 0;
        for (int l = 0; l < NLT; ++l) if (C.l_blk_fill[l] == 0xffff) C.nidle_line++;
        for (int q = 0; q < NBT; ++q) if (C.b_lane_fill[q] == 0xffff) C.nidle_bus_s[q / ROWL]++;
        if (verbose()) {
            long cyc = 0;
            for (int t = 0; t < NLT / ROWL; ++t) cyc += fill_slot_cost(C.l_blk_fill + ROWL * t);
            for (int t = 0; t < NBT / ROWL; ++t) cyc += fill_slot_cost(boff.data() + ROWL * t);
            fprintf(stderr, "relmc: order %d: %d fill blocks: %d cleared by line-slot lanes, %d by bus-slot lanes, %d by the loop; modelled LDS cycles of the block stores %ld\n", order_variant, (int)C.nzero, nline, nbus, nres, cyc);
        }
        return RELMC_OK;
    }

    void base_connectivity()       // is the intact network connected?  (lets the kernel skip the island search when no line is out)
    {
        std::vector<int> lab(nb); for (int i = 0; i < nb; ++i) lab[i] = i;
        auto find = [&](int x) { while (lab[x] != x) { lab[x] = lab[lab[x]]; x = lab[x]; } return x; };
        for (int l = 0; l < nl; ++l) { const int a2 = find(d->br_from[l]), b2 = find(d->br_to[l]); if (a2 != b2) lab[a2] = b2; }
        int roots = 0; for (int i = 0; i < nb; ++i) if (find(i) == i) roots++;
        C.base_connected = roots == 1 ? 1 : 0;
    }

    void thresholds()             // Bernoulli thresholds: fail iff draw_u32 < floor(U * 2^32)   (mc_sampling.m:35, strict '<')
    {
        for (int k = 0; k < ncomp; ++k) {
            double t = std::floor(d->unavail[k] * 4294967296.0);
            if (!(t > 0)) t = 0;
            if (t > 4294967295.0) t = 4294967295.0;
            C.thr[k] = d->always_up[k] ? 0u : (uint32_t)t;   // mc_sampling.m:40-41
        }
    }
    // ---- launch geometry: dynamic LDS = case tables + schedule + one workspace per scenario row
    int geometry()
    {
        const uint32_t case_bytes = (uint32_t)offsetof(DevCaseT<TL>, task);     // tables copied to LDS; the pass schedule is read from global memory
        const uint32_t lds_bytes = 128u + ((case_bytes + 15u) & ~15u) + (uint32_t)SPW * WPB * stride * (uint32_t)sizeof(double) + (ROWL == 16 ? (1024u + 64u) * WPB : 0u);   // + sampling window of the fused path   // 128: solver options
        if (lds_bytes > 160u * 1024u) return failx(RELMC_ERR_UNSUPPORTED, "relmc_case_load: case needs more than 160 KiB of LDS per workgroup");
        geom.stash_off = stash_off; geom.scen_doubles = stride; geom.lds_bytes = lds_bytes;
        return RELMC_OK;
    }
};

}  // namespace

// Build the device tables from the plain case description: internal bus numbering = elimination
// order of the sparse block LDL' (level-then-min-fill, reference bus last), symbolic fill, the
// static task schedule the kernel interprets, incidence lists, thresholds.
// Pure host arithmetic: relmc_debug_symbolic runs it without a device, which is how the CPU test suite checks every schedule it
// produces by interpreting it against a dense solve (tests/test_schedule.py).
template <class TL>
int case_symbolic(const relmc_case_desc* d, DevCaseT<TL>& C, int order_variant, const SymOpts& so, SymGeom& geom, std::string& err)
{
    using S = Symbolic<TL>;
    using clock = std::chrono::steady_clock;
    auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    S s(d, C, order_variant, so, geom, err);
    auto run = [&](std::initializer_list<int (S::*)()> steps) { for (auto step : steps) if (const int rc = (s.*step)()) return rc; return (int)RELMC_OK; };
    if (const int rc = run({&S::header, &S::elimination_order, &S::block_layout, &S::task_list})) return rc;      // the steps that can refuse the case return a code
    const auto t_sched0 = clock::now();
    s.dependencies();
    if (const int rc = s.schedule()) return rc;
    const auto t_place0 = clock::now();
    if (verbose()) fprintf(stderr, "relmc: scheduling %.1f ms\n", ms(t_sched0, t_place0));
    s.place();
    if (verbose()) fprintf(stderr, "relmc: placement search %.1f ms\n", ms(t_place0, clock::now()));
    s.pass_forms();
    s.byte_offsets();
    if (const int rc = run({&S::shadow_idle_lanes, &S::pass_counts, &S::lines, &S::injections})) return rc;
    s.bus_lanes();
    if (const int rc = s.fill_lanes()) return rc;
    s.base_connectivity();
    s.thresholds();
    return s.geometry();
}

template int case_symbolic<Tile24>(const relmc_case_desc*, DevCaseT<Tile24>&, int, const SymOpts&, SymGeom&, std::string&);
template int case_symbolic<Tile96>(const relmc_case_desc*, DevCaseT<Tile96>&, int, const SymOpts&, SymGeom&, std::string&);

// what the solver phase of one Newton step costs under a schedule: its LDS instructions (a pass costs them whatever its fill) + kPassWeight
// per dependent pass (the update passes are LDS-pipe-bound, and every pass is one more wait on the wavefront's chain)
constexpr long kPassWeight = 4;
template <class TL>
long schedule_cost(const DevCaseT<TL>& C, int32_t* lds_out, int32_t* passes_out)
{
    const int nbwd = (int)C.npass - (int)C.npass_upd - (int)C.npass_inv;
    const int nfull = (int)C.npass_upd - (int)C.npass_updh - (int)C.npass_updq;
    long lds = 10L * nfull + 7L * C.npass_updh + 6L * C.npass_updq + 6L * C.npass_inv;
    for (int k = 0; k < nbwd; ++k) lds += (k < 64 && ((C.bwd_half >> k) & 1ull)) ? 6 : 7;
    if (lds_out) *lds_out = (int32_t)lds;
    if (passes_out) *passes_out = (int32_t)C.npass;
    return lds + kPassWeight * (long)C.npass;
}
template <class TL>
int tune_order_impl(const relmc_case_desc* d, DevCaseT<TL>& C, int32_t evaluations, uint64_t seed, const int32_t* start, int32_t* order_out, int32_t* stats)
{
    const int nb = d->nb;
    SymOpts so = sym_opts_default();
    so.place_moves = 0;                                 // the cost does not depend on the operand placement
    std::string err;
    SymGeom g;
    std::vector<int32_t> cur(nb), best(nb), cand(nb);
    int32_t lds = 0, np = 0;
    if (start) cur.assign(start, start + nb);
    else {                                              // the rule's order: external buses by internal number
        const int rc = case_symbolic<TL>(d, C, 0, so, g, err);
        if (rc) return rc;
        for (int e = 0; e < nb; ++e) cur[C.b_int[e]] = e;
    }
    auto eval = [&](const std::vector<int32_t>& o, int32_t* l, int32_t* p) -> long {
        so.order_hint = o.data(); so.n_hint = (int)o.size();
        if (case_symbolic<TL>(d, C, 0, so, g, err) != RELMC_OK) return 1L << 40;      // too much fill / too many passes for the tile: never accepted
        return schedule_cost(C, l, p);
    };
    long cc = eval(cur, &lds, &np);
    if (cc >= (1L << 40)) return RELMC_ERR_INVALID;     // a start order that is not a permutation with the reference bus last, or does not fit
    if (stats) { stats[0] = lds; stats[1] = np; }
    long bc = cc; best = cur; int32_t blds = lds, bnp = np;
    uint64_t rng = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    auto rnd = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    auto unif = [&]() { return (double)(rnd() >> 11) * (1.0 / 9007199254740992.0); };
    double T = 1.2; int since = 0;
    for (int it = 0; it < evaluations && nb > 2; ++it) {
        const int i = (int)(rnd() % (uint64_t)(nb - 1)), j = (int)(rnd() % (uint64_t)(nb - 1));       // the reference bus stays last
        if (i == j) continue;
        cand = cur;
        if (unif() < 0.5) std::swap(cand[i], cand[j]);
        else { const int32_t v = cand[i]; cand.erase(cand.begin() + i); cand.insert(cand.begin() + j, v); }
        int32_t l2 = 0, p2 = 0;
        const long nc = eval(cand, &l2, &p2);
        if (nc <= cc || unif() < std::exp((double)(cc - nc) / T)) {
            cur = cand; cc = nc;
            if (nc < bc) { bc = nc; best = cand; blds = l2; bnp = p2; since = 0; }
        }
        T = T * 0.9995 > 0.12 ? T * 0.9995 : 0.12;
        if (++since > 1500) { cur = best; cc = bc; since = 0; }                                         // back to the best order found so far
    }
    for (int k = 0; k < nb; ++k) order_out[k] = best[k];
    if (stats) { stats[2] = blds; stats[3] = bnp; }
    return RELMC_OK;
}

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

int32_t relmc_tune_order(const relmc_case_desc* d, int32_t evaluations, uint64_t seed, const int32_t* start, int32_t* order_out, int32_t stats_out[4])
{
    if (!d || !order_out || evaluations < 0 || d->nb < 1) return RELMC_ERR_INVALID;
    return with_case_tile(fits_tile24(d), [&](auto& C) { return tune_order_impl(d, C, evaluations, seed, start, order_out, stats_out); });
}

// Host-only introspection (no device, no context): the symbolic analysis and static solver schedule relmc_case_load would build for this
// case under elimination order `order_variant` (0 = primary).  tests/test_schedule.py interprets the schedule on the CPU against a dense
// solve, which is how every ordering / scheduling change is checked before it reaches a GPU.
//   hdr[24]: tile (0 = 16-lane rows, 1 = 64-lane rows), RW, nb, noff, nws, off_rhs, npass, npass_upd, npass_inv, npass_updh, npass_updq,
//            nzero, scen_doubles, lds_bytes, modelled LDS conflict cycles before / after the placement search, MAXPASS, nl, flags, bwd_half (2), longest line / injection
//            list per bus slot (4 bytes), 2 spare
//   tasks[npass][RW][4] (0xffff = no task), pass_ntask[npass], b_int[nb] (external -> internal bus), l_blk[nl] (W offset of the owner
//   line's block, 0xffff otherwise), l_info[nl] (from | to << 8 | flags << 24, internal bus numbers), zero_off[nzero]
int32_t relmc_debug_symbolic(const relmc_case_desc* d, int32_t order_variant, const int32_t* order_hint, int32_t n_hint, int32_t* hdr, uint16_t* tasks, int64_t tasks_cap, uint8_t* pass_ntask,
                             uint8_t* b_int, uint16_t* l_blk, uint32_t* l_info, uint16_t* zero_off, char* err, int32_t err_cap, int32_t model_leaf_free)
{
    if (!d || !hdr || !tasks || !pass_ntask || !b_int || !l_blk || !l_info || !zero_off) return RELMC_ERR_INVALID;
    SymOpts so = sym_opts_default();
    if (order_hint && n_hint > 0) { so.order_hint = order_hint; so.n_hint = n_hint; }
    if (model_leaf_free >= 0) so.model_leaf_free = model_leaf_free;
    std::string errs;
    SymGeom g;
    const int rc = with_symbolic(d, order_variant, so, g, errs, [&](const auto& C) {
        constexpr int rw = std::decay_t<decltype(C)>::ROWL;
        for (int k = 0; k < 24; ++k) hdr[k] = 0;
        hdr[0] = rw == 16 ? 0 : 1; hdr[1] = rw; hdr[2] = C.nb; hdr[3] = C.noff; hdr[4] = (int)C.nws; hdr[5] = C.off_rhs; hdr[6] = C.npass; hdr[7] = C.npass_upd;
        hdr[8] = C.npass_inv; hdr[9] = C.npass_updh; hdr[10] = C.npass_updq; hdr[11] = C.nzero; hdr[12] = (int)g.scen_doubles; hdr[13] = (int)g.lds_bytes;
        hdr[14] = (int)g.conflict_before; hdr[15] = (int)g.conflict_after; hdr[16] = std::decay_t<decltype(C)>::MAXPASS; hdr[17] = C.nl;
        hdr[19] = (int32_t)(uint32_t)(C.bwd_half & 0xffffffffull); hdr[20] = (int32_t)(uint32_t)(C.bwd_half >> 32);
        hdr[21] = (int32_t)((uint32_t)C.maxdeg_s[0] | ((uint32_t)C.maxdeg_s[1] << 8) | ((uint32_t)C.maxinj_s[0] << 16) | ((uint32_t)C.maxinj_s[1] << 24));   // longest line / injection list per bus slot
        if ((int64_t)C.npass * rw * 4 > tasks_cap) return (int)RELMC_ERR_INVALID;
        for (int p = 0; p < C.npass; ++p) { pass_ntask[p] = C.pass_ntask[p]; for (int r = 0; r < rw; ++r) for (int k = 0; k < 4; ++k) {
            // back to offsets in doubles (what tests/schedule_interp.py executes); bit 15 of field 0 of a full-form update pass is the rhs flag
            const uint16_t v = C.task[p][r][k];
            const bool full_upd = p < C.npass_upd - C.npass_updh - C.npass_updq;
            const bool inv = p >= C.npass_upd && p < C.npass_upd + C.npass_inv;
            // idle lanes shadow an active lane in the device image (relmc_debug_task_image); here they stay "no task"
            tasks[((size_t)p * rw + r) * 4 + k] = task_idle(C.task[p][r], inv) ? (uint16_t)0xffff : (uint16_t)((k == 0 && full_upd) ? (((v & 0x7fffu) >> 3) | (v & 0x8000u)) : (v >> 3));
        } }
        for (int i = 0; i < C.nb; ++i) b_int[i] = C.b_int[i];
        for (int l = 0; l < C.nl; ++l) { l_info[l] = C.l_info[l]; l_blk[l] = ((C.l_info[l] >> 24) & LF_OWNER) ? C.l_blk[l] : (uint16_t)0xffff; }
        for (int z = 0; z < C.nzero; ++z) zero_off[z] = C.zero_off[z];
        return (int)RELMC_OK;
    });
    if (err && err_cap > 0) { std::strncpy(err, errs.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return rc;
}

// Host-only introspection: the pass descriptors exactly as the device gets them (byte offsets, idle lanes shadowing an active lane and
// carrying the idle marker; relmc_dev.h).  Same case / order arguments as relmc_debug_symbolic.
//   hdr[16]: tile, RW, nb, nws, off_rhs, npass, npass_upd, npass_inv, npass_updh, npass_updq, bwd_half (2), scen_doubles, modelled LDS
//            conflict cycles of the image with the idle lanes masked / shadowing / masked but every task reading both rows (full form)
//   tasks[npass][RW][4]
int32_t relmc_debug_task_image(const relmc_case_desc* d, int32_t order_variant, const int32_t* order_hint, int32_t n_hint, int32_t* hdr, uint16_t* tasks, int64_t tasks_cap,
                               char* err, int32_t err_cap)
{
    if (!d || !hdr || !tasks) return RELMC_ERR_INVALID;
    SymOpts so = sym_opts_default();
    if (order_hint && n_hint > 0) { so.order_hint = order_hint; so.n_hint = n_hint; }
    std::string errs;
    SymGeom g;
    const int rc = with_symbolic(d, order_variant, so, g, errs, [&](const auto& C) {
        constexpr int rw = std::decay_t<decltype(C)>::ROWL;
        for (int k = 0; k < 16; ++k) hdr[k] = 0;
        hdr[0] = rw == 16 ? 0 : 1; hdr[1] = rw; hdr[2] = C.nb; hdr[3] = (int)C.nws; hdr[4] = C.off_rhs; hdr[5] = C.npass; hdr[6] = C.npass_upd; hdr[7] = C.npass_inv;
        hdr[8] = C.npass_updh; hdr[9] = C.npass_updq; hdr[10] = (int32_t)(uint32_t)(C.bwd_half & 0xffffffffull); hdr[11] = (int32_t)(uint32_t)(C.bwd_half >> 32);
        hdr[12] = (int)g.scen_doubles; hdr[13] = (int)g.shadow_masked; hdr[14] = (int)g.shadow_all; hdr[15] = (int)g.shadow_tasks;
        if ((int64_t)C.npass * rw * 4 > tasks_cap) return (int)RELMC_ERR_INVALID;
        for (int p = 0; p < C.npass; ++p) for (int r = 0; r < rw; ++r) for (int k = 0; k < 4; ++k) tasks[((size_t)p * rw + r) * 4 + k] = C.task[p][r][k];
        return (int)RELMC_OK;
    });
    if (err && err_cap > 0) { std::strncpy(err, errs.c_str(), (size_t)err_cap - 1); err[err_cap - 1] = 0; }
    return rc;
}

}  // extern "C"
