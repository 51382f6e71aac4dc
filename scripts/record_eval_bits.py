"""Records tests/golden/eval_bits_rts24.npz, the bytes that tests/test_eval_bits.py compares the evaluation kernel against:
    RELMC_LIB_PATH=<library of the build to record> python scripts/record_eval_bits.py [out.npz]
Run on the device, once, against the build whose results are to be kept (for the shipped record: the parent of the commit that shared the line
slacks' reciprocal and moved the zero records to the slot lanes).  What is evaluated is the test module's own `evaluate`."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from powersystemsreliabilityassessment_amd import api, case24          # noqa: E402
from tests import test_eval_bits                                       # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else test_eval_bits.GOLDEN
eng = api.Engine(case24.rts24(), device=0)
try:
    rec = test_eval_bits.evaluate(eng)
    version = api._lib.load().relmc_version().decode()
finally:
    eng.close()
np.savez_compressed(out, **test_eval_bits.encode(rec))
print("%s: %d arrays, %d bytes raw, %d bytes on disk, library %s (%s)"
      % (out, len(rec), sum(v.nbytes for v in rec.values()), os.path.getsize(out), os.environ.get("RELMC_LIB_PATH", "default"), version))
