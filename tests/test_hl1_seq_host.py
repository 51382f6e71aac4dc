"""HL1 sequential chronology (relmc_hl1_seq) without a GPU: the host model's interval form against the reference's hour loop and the
exact expectations, the C ABI's declarations / exports / struct layouts, and the Python surface that needs no device."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from powersystemsreliabilityassessment_amd import _abi, _lib, hl1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("hl1_seq_model", os.path.join(ROOT, "tests", "tools", "hl1_seq_model.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


M = _model()


def _rts24():
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    return (np.array([g.capacity for g in gens]), np.array([g.mttf for g in gens]), np.array([g.mttr for g in gens]), load.hourly_load)


@pytest.mark.parametrize("start", [M.ALL_UP, M.STATIONARY])
@pytest.mark.parametrize("fleet,chains,years", [("rts24", [0, 7], 2), ("small", [0, 1, 2, 3, 1 << 33], 4)])
def test_interval_form_equals_the_reference_hour_loop(fleet, chains, years, start):
    """(b) == (a): every per-year loss-hour and loss-event count, EUE to 1e-12, with the state carried across years."""
    cap, mttf, mttr, load = _rts24() if fleet == "rts24" else M.small_fleet()
    a = M.interval_model(5, chains, cap, mttf, mttr, load, years, start)
    b = [np.concatenate(x) for x in zip(*[M.literal_chain(5, c, cap, mttf, mttr, load, years, start) for c in chains])]
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_allclose(a[1], b[1], rtol=1e-12, atol=1e-9)
    assert a[0].sum() > 0 and a[2].sum() > 0                       # the chains do see loss hours


def test_model_matches_the_exact_small_fleet_expectations():
    """(a) against (c): stationary LOLE, EUE and loss events per year within 4.5 standard errors (4000 one-year chains)."""
    cap, mttf, mttr, load = M.small_fleet()
    lole, eue, lolf = M.interval_model(2, range(4000), cap, mttf, mttr, load, 1, M.STATIONARY)
    el, ee, ef = M.small_fleet_stationary(cap, mttf, mttr, load)
    for x, e in ((lole, el), (eue, ee), (lolf, ef)):
        assert abs(x.mean() - e) < 4.5 * x.std() / np.sqrt(x.size), (x.mean(), e)
    # the enumeration's LOLE / EUE are the integer-capacity COPT's
    assert (el, ee) == pytest.approx(M.stationary_year(cap.astype(int), mttf, mttr, load), rel=1e-12)


def test_exact_expectations_on_rts24():
    """(c) on RTS-24: the stationary COPT is run_analytical(step_size=1) (9.3941 h/yr, 1176.29 MWh/yr); the first year of an all-UP
    chain lies measurably below it (the fleet starts with no outage)."""
    cap, mttf, mttr, load = _rts24()
    ref = hl1.run_analytical(hl1.rts24_generators(), hl1.rts24_load(), step_size=1.0)
    sl, se = M.stationary_year(cap.astype(int), mttf, mttr, load)
    assert sl == pytest.approx(ref.lole_hours_yr, rel=1e-9) and se == pytest.approx(ref.eue_mwh_yr, rel=1e-9)
    ul, ue = M.all_up_year1(cap.astype(int), mttf, mttr, load)
    assert 9.0 < ul < sl - 0.15 and ue < se


def test_header_declares_and_library_exports_the_sequential_entry_points():
    hdr = open(os.path.join(ROOT, "include", "relmc.h")).read()
    for s in ("relmc_hl1_seq_load", "relmc_hl1_seq"):
        assert re.search(r"\b" + s + r"\s*\(", hdr), s
        assert s in _lib.EXPORTS
    assert "#define RELMC_HL1_START_ALL_UP     0" in hdr and "#define RELMC_HL1_START_STATIONARY 1" in hdr
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.load()
    assert hasattr(L, "relmc_hl1_seq_load") and hasattr(L, "relmc_hl1_seq")


def test_struct_layouts_match_the_mirrors(tmp_path):
    """sizeof / offsetof of relmc_hl1_seq_year / relmc_hl1_seq_acc from the C compiler == the ctypes mirror == julia's LAYOUT_HL1_SEQ."""
    jl = open(os.path.join(ROOT, "julia", "RelMC.jl")).read()
    block = jl[jl.index("const LAYOUT_HL1_SEQ = ["):]
    block = block[:block.index("\n]\n") + 3]
    table = [(m.group(1), int(m.group(2)), [(f, int(o)) for f, o in re.findall(r'\("(\w+)",\s*(\d+)\)', m.group(3))])
             for m in re.finditer(r'\("(relmc_\w+)",\s*(\d+),\s*\[(.*?)\]\)', block)]
    assert [t[0] for t in table] == ["relmc_hl1_seq_year", "relmc_hl1_seq_acc"]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "relmc.h"', 'int main(void) {']
    for name, _, fields in table:
        prog.append(f'printf("{name} %zu", sizeof({name}));')
        prog += [f'printf(" %zu", offsetof({name}, {f}));' for f, _ in fields]
        prog.append('printf("\\n");')
    prog.append('return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in subprocess.check_output([exe], text=True).splitlines()}
    mirror = {"relmc_hl1_seq_year": _abi.Hl1SeqYear, "relmc_hl1_seq_acc": _abi.Hl1SeqAcc}
    for name, size, fields in table:
        assert got[name] == [size] + [o for _, o in fields], name
        assert C.sizeof(mirror[name]) == size and [f for f, _ in fields] == [f for f, _ in mirror[name]._fields_], name
        for f, o in fields:
            assert getattr(mirror[name], f).offset == o, (name, f)


def test_compare_results_table():
    """compare_results: the header and the `%-20s | %-10.4f | %-10.2f | %-10.4f` rows of PowerSystemAdequacy.jl:275-290."""
    rs = [hl1.ReliabilityResult("Analytical", 9.394110356, 1176.2916768, 0.01234),
          hl1.SequentialReliabilityResult("Sequential MC", 9.4, 1180.0, 2.5, lolf_occ_yr=2.0, lold_hours=4.7)]
    assert hl1.compare_results(rs) == (
        "==========================================\n"
        "       METHOD COMPARISON SUMMARY\n"
        "==========================================\n"
        "Method               | LOLE(h/yr) | EUE(MWh)   | Time(s)   \n"
        "------------------------------------------------------------\n"
        "Analytical           | 9.3941     | 1176.29    | 0.0123    \n"
        "Sequential MC        | 9.4000     | 1180.00    | 2.5000    \n"
        "------------------------------------------------------------\n")


def test_run_sequential_mc_rejects_bad_shapes_before_the_device():
    gens, load = hl1.rts24_generators(), hl1.rts24_load()
    with pytest.raises(ValueError):
        hl1.run_sequential_mc(gens, load, 10, chains=3)
    with pytest.raises(ValueError):
        hl1.run_sequential_mc(gens, load, 0)
    with pytest.raises(ValueError):
        hl1.run_sequential_mc(gens, load, 10, start="cold")
