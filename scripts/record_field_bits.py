"""Records tests/golden/field16_bits.npz: the raw output bits of the split-fp16 field kernels (single launch, forward + reverse, density
only) and of k_light16 on the point pool of tests/test_gpu_tiles.py, for tests/test_gpu_field_bits.py to compare later builds with.

GPU box:   python scripts/record_field_bits.py <libdsnerf_hip.so of the PARENT commit> [out.npz]

The library is given by path on purpose: the fixture is the output of the commit a kernel change starts from (build that commit,
keep its library aside), never of the change itself.  What is evaluated is tests/test_gpu_field_bits.py's own record()."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if len(sys.argv) < 2 or not os.path.exists(sys.argv[1]):
    raise SystemExit(__doc__)
os.environ["DSNERF_LIB"] = os.path.abspath(sys.argv[1])          # read by dsnerf_amd._lib when it is first imported
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "field16_bits.npz")
for q in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import numpy as np  # noqa: E402
import test_gpu_field_bits as FB  # noqa: E402

ctx = FB.TT.Ctx()
assert ctx.lib.LIB_PATH == os.environ["DSNERF_LIB"], ctx.lib.LIB_PATH
arrays = FB.record(ctx)
np.savez_compressed(out_path, **arrays)
print("recorded with", ctx.lib.LIB_PATH, "at", subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
      or "(no git)")
for k, a in arrays.items():
    print("  %-22s %-12s nonzero %d" % (k, a.shape, int(np.count_nonzero(a.reshape(len(a), -1).any(1)))))
print(out_path, os.path.getsize(out_path), "bytes")
