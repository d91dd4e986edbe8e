"""Golden vectors for the body model (dsn_body_shape / dsn_body_pose), from the reference's own code: utils/h36m_utils.get_rigid_transformation
and get_bounds, the padding of dataloader/zju_mocap_dataset.Mocap_Base.prepare_input (run on a scratch directory of .npy files, both
modes) and utils/blend_utils.ppts_to_pts in float32 and float64.  cv2 and glob2 are stubbed by empty modules (cv2.Rodrigues, which
prepare_input calls for a value this fixture does not keep, returns the identity).  Arrays only; the recorded bars go to
body_pose_errors.json.  Run in the build container with the reference's checkout as the argument (or in DSN_REFERENCE):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_body_pose.py /path/to/reference"""
import json, os, sys, tempfile, types
import numpy as np
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import dsnerf_amd.synth as synth  # noqa: E402
import body_pose_restate as BP  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("DSN_REFERENCE", "")
assert os.path.isdir(REF), "give the reference's checkout: make_golden_body_pose.py DIR (or DSN_REFERENCE)"
cv2 = types.ModuleType("cv2")
cv2.Rodrigues = lambda r: (np.eye(3), None)
sys.modules["cv2"] = cv2
sys.modules["glob2"] = types.ModuleType("glob2")
sys.path.insert(0, REF)
import importlib.util  # noqa: E402
import torch  # noqa: E402
from utils import blend_utils, h36m_utils  # noqa: E402
# (the module file itself: the package's __init__ pulls in every data set and their image libraries)
_spec = importlib.util.spec_from_file_location("ref_zju_mocap_dataset", os.path.join(REF, "dataloader", "zju_mocap_dataset.py"))
zju_mocap_dataset = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(zju_mocap_dataset)

out, bars = {}, {}

# ---- the joint chain: three parent tables x pose sets (ordinary, zero, beyond pi, 1e-9) ----
joints = ((synth.hash_uniform(72, 911).reshape(24, 3) - np.float32(0.5)) * np.array([1.6, 1.5, 0.3], np.float32)).astype(np.float32)
pose_sets = {
    "poses": np.stack([synth.make_poses(s) for s in (5, 6, 7, 8)]),
    "zero": np.zeros((1, 24, 3), np.float32),
    "beyond_pi": np.stack([(synth.hash_normal(72, s) * np.float32(2.5)).reshape(24, 3) for s in (21, 22)]).astype(np.float32),
    "tiny": np.stack([((synth.hash_uniform(72, s) - np.float32(0.5)) * np.float32(4e-9)).reshape(24, 3) for s in (31, 32)]).astype(np.float32),
}
assert (np.linalg.norm(pose_sets["beyond_pi"], axis=-1) > np.pi).mean() > 0.4
tables = {"smpl": BP.SMPL_PARENTS, "chain": BP.CHAIN_PARENTS, "star": BP.STAR_PARENTS}
out["joints"] = joints
equal, total, worst = 0, 0, 0
for tn, parents in tables.items():
    out[f"parents:{tn}"] = parents
    for pn, poses in pose_sets.items():
        out[f"poses:{pn}"] = poses
        par = parents.astype(np.int64)
        ref = np.stack([h36m_utils.get_rigid_transformation(p.astype(np.float64), joints.astype(np.float64), par) for p in poses])
        assert ref.dtype == np.float32
        out[f"A:{tn}:{pn}"] = ref
        mine = BP.chain(poses, joints, parents)[0]
        ulp = np.abs(mine.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
        ulp = np.where((mine == 0) & (ref == 0), 0, ulp)                  # (+0 and -0 are the same value)
        equal, total, worst = equal + int((ulp == 0).sum()), total + ulp.size, max(worst, int(ulp.max()))
        print(f"A {tn:5s} {pn:9s} bit-equal {float((ulp == 0).mean()):.5f}, worst {int(ulp.max())} ulp")
bars["chain_bit_equal_fraction"] = equal / total
bars["chain_worst_ulp"] = worst
assert worst <= 1 and equal / total >= 0.99, (worst, equal / total)

# ---- bounds: the reference's padding on the restatement's world vertices of the small body ----
canon, _ = synth.make_small_body()
vt, w, Jr, sd, pd = BP.make_model(canon)
vs, jn = BP.shape(vt, sd, (synth.hash_normal(10, 77) * np.float32(0.8)).astype(np.float32), Jr)
clip = np.stack([synth.make_poses(s) for s in (41, 42, 43, 44)])
Rh = (synth.hash_normal(12, 51) * np.float32(0.7)).reshape(4, 3).astype(np.float32)
Th = (synth.hash_normal(12, 52) * np.float32(0.9)).reshape(4, 3).astype(np.float32)
e = BP.pose(vs, jn, BP.SMPL_PARENTS, w, pd, clip, Rh, Th)
out.update({"clip:betas": (synth.hash_normal(10, 77) * np.float32(0.8)).astype(np.float32), "clip:poses": clip, "clip:Rh": Rh, "clip:Th": Th,
            "clip:xyz": e["xyz"], "clip:xyz_smpl": e["xyz_smpl"], "clip:v_posed": e["v_posed"], "clip:A": e["A"]})
ds = object.__new__(zju_mocap_dataset.Mocap_Base)
with tempfile.TemporaryDirectory() as tmp:
    ds.vertices_dir, ds.smpl_dir, ds.use_x_pose = os.path.join(tmp, "v"), os.path.join(tmp, "p"), False
    os.makedirs(ds.vertices_dir), os.makedirs(ds.smpl_dir)
    for i in range(4):
        np.save(os.path.join(ds.vertices_dir, f"{i}.npy"), e["xyz"][i])
        np.save(os.path.join(ds.smpl_dir, f"{i}.npy"), {"Rh": Rh[i:i + 1], "Th": Th[i:i + 1], "poses": clip[i].reshape(1, 72)}, allow_pickle=True)
    for mode, key in (("train", "zju_train"), ("test", "zju_eval")):
        ds.mode = mode
        got = np.stack([ds.prepare_input(i)[2] for i in range(4)])
        assert got.dtype == np.float32
        out[f"bounds:{key}"] = got
out["bounds:h36m"] = np.stack([h36m_utils.get_bounds(e["xyz"][i]) for i in range(4)])

# ---- the round trip through the reference: ppts_to_pts(xyz_smpl, weights, A) in float32, and its float64 run on the same inputs ----
t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
args = lambda dt: (t(e["xyz_smpl"], dt), t(np.broadcast_to(w.T[None], (4, 24, w.shape[0])), dt), t(e["A"], dt))  # noqa: E731
z32 = blend_utils.ppts_to_pts(*args(torch.float32)).numpy()
z64 = blend_utils.ppts_to_pts(*args(torch.float64)).numpy()
out["clip:ppts_to_pts"] = z32
bars["ppts_to_pts_f32_vs_f64"] = float(np.abs(z32.astype(np.float64) - z64).max())
bars["round_trip_achieved"] = float(np.abs(z32.astype(np.float64) - e["v_posed"].astype(np.float64)).max())
print(bars)
np.savez_compressed(os.path.join(HERE, "body_pose.npz"), **out)
with open(os.path.join(HERE, "body_pose_errors.json"), "w") as f:
    json.dump(bars, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote body_pose.npz", os.path.getsize(os.path.join(HERE, "body_pose.npz")), "bytes")
