"""No GPU: the host side of the device-resident evaluation (eval_device's layouts and readers, train.py's periodic_eval gate)."""
import importlib.util
import os
import types

import numpy as np
import pytest

from tests import eval_cases as EC
from unsupervised_depth_opticalflow_egomotion_amd import eval_device as ED

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _driver(name):
    spec = importlib.util.spec_from_file_location("dfe_%s_driver" % name, os.path.join(REPO, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _train_module():
    return _driver("train")


@pytest.mark.parametrize("hw", [(375, 1242), (370, 1226), (37, 61), (40, 64)])
def test_crop_box_is_the_references_int32_truncation(hw):
    h, w = hw
    ref = np.array([0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w]).astype(np.int32)
    assert ED.crop_box(h, w) == tuple(int(v) for v in ref)
    host = ED.pack_depth_gt([np.full(hw, 5.0, np.float32)])
    assert host["dims"].dtype == np.int32 and host["dims"][0].tolist() == [h, w] + [int(v) for v in ref]


def test_flag_plane_and_padded_layout_round_trip():
    gts, nocs, movs, _ = EC.flow_case((16, 32))
    host = ED.pack_flow_gt(gts, nocs, movs)
    hmax, wmax = max(s[0] for s in EC.GT_SIZES), max(s[1] for s in EC.GT_SIZES)
    assert host["u"].shape == (5, hmax, (wmax + 3) // 4 * 4) and host["u"].shape[2] % 4 == 0
    assert host["flags"].dtype == np.uint8 and host["dims"].tolist() == [list(s) for s in EC.GT_SIZES]
    us, vs, fs = (ED.unpad_planes(host[k], host["dims"]) for k in ("u", "v", "flags"))
    for i, gt in enumerate(gts):
        valid, noc, mv = ED.unpack_flags(fs[i])
        assert np.array_equal(us[i], gt[:, :, 0]) and np.array_equal(vs[i], gt[:, :, 1])
        assert np.array_equal(valid, gt[:, :, 2]) and np.array_equal(noc, nocs[i]) and np.array_equal(mv, movs[i])
        assert not host["u"][i, gt.shape[0]:].any() and not host["flags"][i, :, gt.shape[1]:].any()      # the padding is zero
    assert gts[0][3, 5, 2] == 0 and nocs[0][3, 5] == 1 and fs[0][3, 5] == ED.FLAG_NOC                    # noc without valid survives
    without = ED.pack_flow_gt(gts, nocs)
    assert not (without["flags"] & ED.FLAG_MOVING).any()
    with pytest.raises(ValueError, match="other than 0 and 1"):
        ED.pack_flags(np.array([[0.5]]), np.array([[0.0]]))
    gd, _ = EC.depth_case((16, 32), "uniform")
    hd = ED.pack_depth_gt(gd)
    assert all(np.array_equal(a, b) for a, b in zip(ED.unpad_planes(hd["gt"], hd["dims"]), gd))


def test_sets_find_the_samples_of_a_miniature_tree(tmp_path):
    from unsupervised_depth_opticalflow_egomotion_amd import kitti_io as K
    cfg = EC.mini_tree(str(tmp_path))
    for year in (2012, 2015):
        gt_dir = getattr(cfg, "gt_%d_dir" % year)
        s = ED.FlowEvalSet.from_kitti(gt_dir, cfg.img_hw, year)
        assert len(s) == 3 and s.has_moving == (year == 2015) and tuple(s.inputs.shape) == (3, 3, 128, 128)
        assert s.dims.tolist() == [[40, 136], [38, 132], [40, 136]] and (s.hmax, s.wmax) == (40, 136)
        gts, nocs = K.load_gt_flow_kitti(gt_dir, "kitti_%d" % year, 3)
        assert np.array_equal(s.u[1, :38, :132].numpy(), gts[1][:, :, 0].astype(np.float32))
        assert np.array_equal(ED.unpack_flags(s.flags[1, :38, :132].numpy())[1], nocs[1].astype(np.float32))
        pairs = K.KITTIFlowPairs(gt_dir, cfg.img_hw, 3, year)
        assert bool((s.inputs[2] == pairs[2][0]).all())                      # the bits test.py's task feeds the nets
    d = ED.DepthEvalSet.from_eigen(cfg.raw_base_dir, cfg.eigen_dir, cfg.img_hw)
    assert len(d) == 3 and tuple(d.inputs.shape) == (3, 3, 64, 128) and d.dims[:, :2].tolist() == [[40, 136], [38, 132], [40, 136]]
    img = K.read_image_bgr(os.path.join(cfg.raw_base_dir, "2011_09_26/drive_0001/image_02/data/%010d.png" % 1))
    x = (K.resize_bilinear_u8(img, cfg.img_hw) / 255.0).astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(d.inputs[1].numpy(), x)
    with pytest.raises(FileNotFoundError):
        ED.FlowEvalSet.from_kitti(str(tmp_path / "nothing"), cfg.img_hw, 2012)


def test_an_empty_depth_mask_raises_naming_the_sample():
    good = np.full((37, 61), 5.0, np.float32)
    empty = np.zeros((37, 61), np.float32)
    empty[0, 0] = 5.0          # outside the crop box
    empty[20, 20] = 90.0       # inside it, beyond max_depth
    with pytest.raises(ValueError, match="sample 1 .*mask is empty"):
        ED.DepthEvalSet([good, empty])
    with pytest.raises(ValueError, match="drive_7 0000000003"):
        ED.DepthEvalSet([empty], names=["drive_7 0000000003"])


def test_mode_to_task_mapping():
    assert ED.tasks_for_mode("flow") == ("flow_2012", "flow_2015")
    assert ED.tasks_for_mode("depth") == ("depth",)
    assert ED.tasks_for_mode("geom") == ("flow_2012", "flow_2015", "depth")
    assert [ED.RESULT_KEYS[t] for t in ED.tasks_for_mode("geom")] == ["eval_2012_res", "eval_2015_res", "eval_eigen_res"]
    with pytest.raises(ValueError):
        ED.tasks_for_mode("pose")


def test_periodic_eval_gate_and_build_evaluator_without_data(tmp_path):
    T = _train_module()

    class Boom:
        def run(self):
            raise AssertionError("the evaluator must not run")
    logs = []
    cfg = types.SimpleNamespace(no_test=True, test_interval=1, model_dir=str(tmp_path))
    assert T.periodic_eval(cfg, Boom(), 0, logs) is None                       # --no_test
    cfg.no_test = False
    assert T.periodic_eval(cfg, None, 0, logs) is None                         # no evaluator: the config names no data
    cfg.test_interval = 5
    assert T.periodic_eval(cfg, Boom(), 3, logs) is None                       # off the interval
    assert logs == [] and not os.path.exists(os.path.join(str(tmp_path), "log.pkl"))
    # the shipped config names none of the directories: nothing is built, whatever the mode
    import yaml
    with open(os.path.join(REPO, "config", "kitti_geom.yaml")) as fh:
        shipped = T.merge_cfg(T.build_parser().parse_args([]), yaml.safe_load(fh))
    ns = types.SimpleNamespace(**shipped)
    assert T.build_evaluator(ns, None, None) is None
    ns.no_test = True
    assert T.build_evaluator(ns, None, None) is None


def test_fused_eval_refuses_a_result_dir(monkeypatch, tmp_path):
    """test.py --fused_eval keeps no per-image prediction on the host: with --result_dir it raises before anything is loaded"""
    drv = _driver("test")
    monkeypatch.setattr("sys.argv", ["test.py", "--task", "kitti_depth", "--fused_eval", "--result_dir", str(tmp_path / "out")])
    with pytest.raises(ValueError, match="--fused_eval"):
        drv.main()
    assert not os.path.exists(str(tmp_path / "out"))
    monkeypatch.setattr("sys.argv", ["test.py", "--task", "kitti_pose", "--fused_eval"])
    with pytest.raises(ValueError, match="kitti_pose"):
        drv.main()


def test_conditioned_inputs_leave_no_decision_in_the_band():
    """the builders of the GPU tests' inputs: cheap enough to check here as well"""
    for hw in EC.PRED_SIZES:
        gts, _, _, preds = EC.flow_case(hw)
        assert sum(int(EC.flow_near(g, p, hw).sum()) for g, p in zip(gts, preds)) == 0
        for kind in ("uniform", "constant", "span"):
            gd, dd = EC.depth_case(hw, kind)
            counts = [int(EC.depth_near(g, d)[1].sum()) for g, d in zip(gd, dd)]
            assert sum(int(EC.depth_near(g, d)[0].sum()) for g, d in zip(gd, dd)) == 0
            assert counts[0] % 2 == 1 and counts[1] % 2 == 0 and counts[1] > 2 and counts[2] == 1 and counts[3] == 2 and counts[4] > 100
