"""`scripts/eval_sharded.py --data-dir DIR --smpl-dir SMPL_DIR` on the synthetic 3DPW-format directory of tests/golden/pw3d_files.py (two
genders) and two seeded synthetic SMPL models written as .npz: MPVPE is a number, and it is the number this process gets from the same
model's predictions against `FrameTable.gt_mesh` through `Evaluator.per_sample` with the SMPL root row."""
import json
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest
import torch

import smpl_ref as SR

pytestmark = pytest.mark.gpu
HERE = osp.dirname(osp.abspath(__file__))
REPO = osp.dirname(HERE)


def test_eval_sharded_reports_mpvpe_from_the_smpl_fits(tmp_path):
    from pmce_amd import assets, datasets, models, smpl, synth
    from pmce_amd.eval import Evaluator
    sys.path.insert(0, osp.join(HERE, "golden"))
    import pw3d_files
    path = pw3d_files.write(str(tmp_path))
    sdir = tmp_path / "smpl"
    sdir.mkdir()
    kt = np.stack([np.array(SR.PARENTS, dtype=np.uint32), np.arange(24, dtype=np.uint32)])
    for k, g in enumerate(("male", "female")):
        m = SR.synthetic_model(6890, SR.SEED + 20 + k)
        np.savez(sdir / (smpl.MODEL_FILES[g] + ".npz"), kintree_table=kt, f=m["faces"],
                 **{key: m[key].astype(np.float32) for key in ("v_template", "shapedirs", "posedirs", "weights", "J_regressor")})
    env = dict(os.environ, PMCE_SYNTHETIC_BASE_DATA="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, osp.join(REPO, "scripts", "eval_sharded.py"), "--data-dir", path, "--smpl-dir", str(sdir), "--batch", "32"],
                       env=env, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert got["samples"] == 67 and isinstance(got["MPVPE"], float) and np.isfinite(got["MPVPE"]) and got["MPVPE"] > 0
    assert "SMPL fits" in got["data"] and "void" not in got["data"]
    # the flag without the files it works on is an error, not a silent no-op
    bad = subprocess.run([sys.executable, osp.join(REPO, "scripts", "eval_sharded.py"), "--smpl-dir", str(sdir)], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--data-dir" in bad.stderr

    # the same in this process
    assets.allow_synthetic_base_data()
    dev = torch.device("cuda:0")
    table = datasets.load_pw3d(path)
    assert set(table.smpl["gender"]) == {"male", "female"}
    win = table.windows()
    mid = datasets.window_mid(win)
    layer = smpl.SMPL.from_dir(str(sdir))
    model = models.PMCE.get_model(19, 256, 3)
    model.load_state_dict(synth.make_state_dict(synth.pmce_spec(19, 256, 3), seed=123))
    model = model.to(dev)
    mesh = model(*datasets.window_batch(table.pose2d(dev), table.features_on(dev), win))[0]
    ev = Evaluator(dev, root_regressor_row=layer.root_regressor_row())
    gj = torch.from_numpy(table.gt_joints_root_relative()[mid]).to(dev)
    mv = ev.per_sample(mesh, table.gt_mesh(layer, mid, dev), gj)[0].double().mean().item()
    print(f"eval_sharded MPVPE {got['MPVPE']:.4f} mm, in process {mv:.4f} mm")
    # fp32 per-sample errors of a few hundred mm summed in fp64: other batch boundaries change nothing but the forward's batch size
    assert abs(got["MPVPE"] - mv) < 2e-3 * max(1.0, mv / 100)
