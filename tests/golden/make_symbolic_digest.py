"""Writes tests/golden/symbolic_image_digest.json: per case one SHA-256 over everything `relmc_debug_symbolic` writes (header and arrays)
and one over everything `relmc_debug_task_image` writes, or the return code where the library refuses the case.  The cases are the
default-option ones of profiles/symbolic_steps: RTS-24 / RTS-96 under the rule's three orders and under their shipped order, and the
random networks of tests/test_schedule.py and tests/test_pass_shadow.py under all three.  tests/test_schedule.py recomputes them.
No GPU.  Usage: python tests/golden/make_symbolic_digest.py   (RELMC_LIB_PATH selects the library, as everywhere)"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from powersystemsreliabilityassessment_amd import _abi, case24, case96         # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "symbolic_image_digest.json")
# (seed, buses, chords, generators, load buses): tests/test_schedule.py::test_random_networks, then seeds 8 and 9 of tests/test_pass_shadow.py
RANDOM = [(1, 2, 0, 2, 1), (2, 7, 3, 4, 4), (3, 19, 8, 9, 10), (4, 30, 14, 12, 14), (5, 60, 25, 30, 35), (6, 100, 26, 40, 50), (7, 120, 6, 40, 60),
          (8, 5, 2, 3, 3), (9, 9, 3, 4, 4)]


def cases():
    """(name, case, order variant, order hint or None), in the fixture's order"""
    from tests.test_random_cases import random_case
    out = []
    for name, case in (("rts24", case24.rts24()), ("rts96", case96.rts96())):
        out += [(f"{name}/rule/{v}", case, v, None) for v in (0, 1, 2)]
        out.append((f"{name}/shipped/0", case, 0, case.elim_order))
    for seed, nb, chords, ng, loads in RANDOM:
        case = random_case(np.random.default_rng(100 + seed), nb, chords, ng, loads)
        out += [(f"random{seed}_{nb}/rule/{v}", case, v, None) for v in (0, 1, 2)]
    return out


def digest(L, case, variant, order):
    """{"rc": code} where the library refuses the case, else the two digests"""
    vp = C.c_void_p
    L.relmc_debug_symbolic.restype = C.c_int32
    L.relmc_debug_symbolic.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, C.c_int64, vp, vp, vp, vp, vp, C.c_char_p, C.c_int32, C.c_int32]
    L.relmc_debug_task_image.restype = C.c_int32
    L.relmc_debug_task_image.argtypes = [vp, C.c_int32, vp, C.c_int32, vp, vp, C.c_int64, C.c_char_p, C.c_int32]
    holder = _abi.CaseHolder(case)
    hint = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    hp, hn = (None, 0) if hint is None else (hint.ctypes.data, int(hint.size))
    err = C.create_string_buffer(512)
    sym = [np.zeros(24, np.int32), np.zeros(96 * 64 * 4, np.uint16), np.zeros(96, np.uint8), np.zeros(256, np.uint8), np.zeros(256, np.uint16),
           np.zeros(256, np.uint32), np.zeros(512, np.uint16)]
    rc = L.relmc_debug_symbolic(C.byref(holder.desc), variant, hp, hn, sym[0].ctypes.data, sym[1].ctypes.data, sym[1].size, *[a.ctypes.data for a in sym[2:]],
                                err, 512, -1)
    img = [np.zeros(16, np.int32), np.zeros(96 * 64 * 4, np.uint16)]
    rc2 = L.relmc_debug_task_image(C.byref(holder.desc), variant, hp, hn, img[0].ctypes.data, img[1].ctypes.data, img[1].size, err, 512)
    if rc != 0 or rc2 != 0:
        assert rc == rc2, (rc, rc2)
        return {"rc": int(rc)}
    sha = lambda arrays: hashlib.sha256(b"".join(a.tobytes() for a in arrays)).hexdigest()      # the whole zero-initialised buffers: whatever is written
    return {"rc": 0, "symbolic": sha(sym), "task_image": sha(img)}


def main():
    from powersystemsreliabilityassessment_amd import _lib
    L = _lib.load()
    out = {name: digest(L, case, variant, order) for name, case, variant, order in cases()}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(f"{len(out)} cases, {sum(1 for v in out.values() if v['rc'] != 0)} refused by the library")


if __name__ == "__main__":
    main()
