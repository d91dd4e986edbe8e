"""Records tests/golden/train_grad_bits.json: SHA-256, float64 sum and L2 norm of the trunk's parameter gradients (names containing
`stage`) of the cases of tests/test_gpu_train_bits.py, for that module to compare later builds with.

GPU box:   python scripts/record_train_bits.py <libdsnerf_hip.so of the PARENT commit> [out.json]

The library is given by path on purpose: the fixture is the output of the commit a change of the training step starts from (build
that commit, keep its library aside), never of the change itself.  Each case runs twice, each time in a child process of its own with
the default environment (tests/_grads_dump.py, as test_gpu_round5.py runs it); nothing is written unless the two processes agree bit
for bit on every trunk tensor of every case."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if len(sys.argv) < 2 or not os.path.exists(sys.argv[1]):
    raise SystemExit(__doc__)
lib_path = os.path.abspath(sys.argv[1])
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "train_grad_bits.json")
for q in (os.path.join(ROOT, "oracle"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, q)
import numpy as np  # noqa: E402
import test_gpu_train_bits as TB  # noqa: E402

env = {k: v for k, v in os.environ.items() if not k.startswith("DSN_")}          # the default environment: no switch set
env["DSNERF_LIB"] = lib_path                                                      # read by dsnerf_amd._lib when it is first imported
cases, refused = {}, []
with tempfile.TemporaryDirectory() as tmp:
    for name in TB.CASES:
        runs = []
        for k in range(2):
            path = os.path.join(tmp, "%s_%d.npz" % (name, k))
            p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_grads_dump.py"), name, path], env=env, capture_output=True,
                               text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("%s, process %d: exit %d\n%s" % (name, k, p.returncode, p.stderr[-2000:]))
            with np.load(path) as z:
                runs.append({key: z[key] for key in z.files if "stage" in key})
        differ = [key for key in runs[0] if not np.array_equal(runs[0][key].view(np.int32), runs[1][key].view(np.int32))]
        print("%-26s %2d trunk tensors, %d differ between the two processes %s" % (name, len(runs[0]), len(differ), differ or ""), flush=True)
        if differ or not runs[0]:
            refused.append((name, differ))
        cases[name] = TB.trunk_digests(runs[0])
if refused:
    raise SystemExit("NOT written: the trunk is not reproducible across processes for %r" % refused)
commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "(no git)"
with open(out_path, "w") as f:
    json.dump({"what": "trunk gradient digests, scripts/record_train_bits.py; two processes per case agreed bit for bit",
               "library": os.path.basename(lib_path), "cases": cases}, f, indent=1, sort_keys=True)
    f.write("\n")
print("recorded with", lib_path, "at", commit)
print(out_path, os.path.getsize(out_path), "bytes")
