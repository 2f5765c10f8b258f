"""GPU: the device-resident KITTI evaluation -- the metric kernels (dfe_eval_flow / dfe_eval_depth, csrc/ops_eval.hip) on synthetic
predictions against oracle/eval_oracle.py, their bits and bounds, and eval_device.Evaluator against test.py's per-image path.

Tolerances are the ones core.evaluation is held to against the same oracle (test_hip_models.py,
test_device_side_evaluation_at_kitti_size): atol = 1.01e-4, rtol = 1e-4 on the flow table, rtol = 3e-5 on the depth metrics.  The
inputs are conditioned (tests/eval_cases.py): no float64 decision lies within a relative 1e-4 of its threshold, and no pixel or
sample is left out of a comparison."""
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

from oracle import eval_oracle as EO
from tests import eval_cases as EC
from tests import guarded as G
from unsupervised_depth_opticalflow_egomotion_amd import convs, eval_device as ED, synthetic
from unsupervised_depth_opticalflow_egomotion_amd._lib import get_lib
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg, make_optimizer, train_step

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 4                       # five samples: a tail batch of one runs
FLOW_TOL = dict(atol=1.01e-4, rtol=1e-4)
DEPTH_TOL = dict(rtol=3e-5)


def dev():
    return torch.device("cuda:0")


def _driver(name):
    spec = importlib.util.spec_from_file_location("dfe_%s_driver" % name, os.path.join(REPO, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flow_pred(preds):
    return torch.from_numpy(np.stack([p.transpose(2, 0, 1) for p in preds])).to(dev()).contiguous()


def _disp(disps):
    return torch.from_numpy(np.stack(disps)[:, None]).to(dev()).contiguous()


def _flow_records(fset, pred):
    n = len(fset)
    rec = torch.empty((n, 16), dtype=torch.float64, device=dev())
    for first in range(0, n, BATCH):
        ED.eval_flow_records(fset, pred[first:first + BATCH], first, rec[first:first + BATCH])
    return rec


def _depth_records(dset, disp):
    n = len(dset)
    rec = torch.empty((n, 10), dtype=torch.float64, device=dev())
    for first in range(0, n, BATCH):
        ED.eval_depth_records(dset, disp[first:first + BATCH], first, rec[first:first + BATCH])
    return rec


def _oracle_pred_depths(gts, disps):
    return [(np.float32(1.0) / (EO.resize_linear(d[:, :, None], g.shape)[:, :, 0] + np.float32(1e-4))).astype(np.float32)
            for g, d in zip(gts, disps)]


# ---------------------------------------------------------------------------------------------------------------- 1, 3: flow
@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("pred_hw", EC.PRED_SIZES)
def test_flow_table_against_the_oracle(pred_hw, moving):
    gts, nocs, movs, preds = EC.flow_case(pred_hw)
    assert sum(int(EC.flow_near(g, p, pred_hw).sum()) for g, p in zip(gts, preds)) == 0          # conditioned, nothing excluded
    assert np.array_equal(gts[1][:, :, 2], nocs[1])                                               # the occ denominator clamp
    assert gts[0][3, 5, 2] == 0 and nocs[0][3, 5] == 1                                            # noc = 1, valid = 0
    assert all(((g[:, :, 0] == 0) & (g[:, :, 1] == 0) & (g[:, :, 2] == 1)).any() for g in gts)    # the 1e-10 clamp
    fset = ED.FlowEvalSet(gts, nocs, movs if moving else None, device=dev())
    rec = _flow_records(fset, _flow_pred(preds))
    table = ED.flow_table(rec, moving).cpu().numpy()
    ref = EO.eval_flow_avg(gts, nocs, preds, pred_hw, movs if moving else None)
    print("\nflow table %s moving=%s\n  kernel %s\n  oracle %s\n  max |diff| %.3e" % (pred_hw, moving, table, ref, np.abs(table - ref).max()))
    np.testing.assert_allclose(table, ref, **FLOW_TOL)       # both in eval_flow_avg's accumulator order
    r = rec.cpu().numpy()
    assert r[1, 7] == 0 and r[0, 7] == (gts[0][:, :, 2] - nocs[0]).sum()                         # sum (valid - noc), arithmetic form
    assert np.array_equal(r[:, 5], [g[:, :, 2].sum() for g in gts]) and np.array_equal(r[:, 6], [m.sum() for m in nocs])
    # the formatted string is evaluation.eval_flow_avg's
    text = ED.format_flow_table(table.tolist(), moving)
    assert text.split("\n")[0].split(",")[-1].strip() == "err_rate" and len(text.split("\n")[1].split(",")) == (8 if moving else 4)


# ---------------------------------------------------------------------------------------------------------------- 2, 3: depth
@pytest.mark.parametrize("kind", ["uniform", "constant", "span"])
@pytest.mark.parametrize("pred_hw", EC.PRED_SIZES)
def test_depth_metrics_against_the_oracle(pred_hw, kind):
    gts, disps = EC.depth_case(pred_hw, kind)
    near = [EC.depth_near(g, d) for g, d in zip(gts, disps)]
    assert sum(int(a.sum()) for a, _ in near) == 0                                                # conditioned, nothing excluded
    counts = [int(m.sum()) for _, m in near]
    assert counts[0] % 2 == 1 and counts[1] % 2 == 0 and counts[2] == 1 and counts[3] == 2
    dset = ED.DepthEvalSet(gts, device=dev())
    rec = _depth_records(dset, _disp(disps)).cpu().numpy()
    preds = _oracle_pred_depths(gts, disps)
    ref = EO.eval_depth(gts, preds)
    got = rec[:, :7].astype(np.float32).mean(0)
    print("\ndepth %s %s counts %s\n  kernel %s\n  oracle %s\n  max rel %.3e" % (pred_hw, kind, counts, got, ref, np.abs(got / ref - 1).max()))
    assert np.array_equal(rec[:, 9], counts)
    np.testing.assert_allclose(got, ref, **DEPTH_TOL)
    for i, (g, p) in enumerate(zip(gts, preds)):                                                  # every sample's medians
        m = near[i][1]
        np.testing.assert_allclose(rec[i, 7], np.median(g[m]), rtol=0, atol=0)                    # ground truth: exact
        np.testing.assert_allclose(rec[i, 8], np.median(p[m]), rtol=1e-6)                         # pred: the fp32 resize's rounding


@pytest.mark.parametrize("kind", ["uniform", "constant", "span"])
def test_depth_medians_bit_for_bit_at_identity_size(kind):
    """h, w == H, W: the resize is the identity and the division correctly rounded, so the select's two medians are numpy's."""
    sizes = ((37, 61),) * 5
    gts, disps = EC.depth_case(None, kind, seed=3, sizes=sizes)
    dset = ED.DepthEvalSet(gts, device=dev())
    rec = _depth_records(dset, _disp(disps)).cpu().numpy()
    for i, (g, d) in enumerate(zip(gts, disps)):
        p = (np.float32(1.0) / (d + np.float32(1e-4))).astype(np.float32)
        m = EC.depth_near(g, d)[1]
        mg, mp = np.median(g[m]), np.median(p[m])
        assert mg.dtype == np.float32 and mp.dtype == np.float32
        assert np.float32(rec[i, 7]).tobytes() == mg.tobytes() and rec[i, 7] == float(mg), (i, rec[i, 7], mg)
        assert np.float32(rec[i, 8]).tobytes() == mp.tobytes() and rec[i, 8] == float(mp), (i, rec[i, 8], mp)
    np.testing.assert_allclose(rec[:, :7].astype(np.float32).mean(0),
                               EO.eval_depth(gts, [(np.float32(1.0) / (d + np.float32(1e-4))).astype(np.float32) for d in disps]), **DEPTH_TOL)


# ---------------------------------------------------------------------------------------------------------------- 4: bits
def test_records_do_not_depend_on_batch_run_or_stream():
    pred_hw = EC.PRED_SIZES[1]
    gts, nocs, movs, preds = EC.flow_case(pred_hw)
    gd, dd = EC.depth_case(pred_hw, "span")
    fset, dset = ED.FlowEvalSet(gts, nocs, movs, device=dev()), ED.DepthEvalSet(gd, device=dev())
    fp, dp = _flow_pred(preds), _disp(dd)
    same = lambda a, b: torch.equal(a.view(torch.int64), b.view(torch.int64))      # noqa: E731
    f4, d4 = ED.eval_flow_records(fset, fp[:4]), ED.eval_depth_records(dset, dp[:4])
    for i in (0, 2, 3):
        assert same(ED.eval_flow_records(fset, fp[i:i + 1], i)[0], f4[i]), i          # alone == inside a batch of four
        assert same(ED.eval_depth_records(dset, dp[i:i + 1], i)[0], d4[i]), i
    assert same(ED.eval_flow_records(fset, fp[:4]), f4) and same(ED.eval_depth_records(dset, dp[:4]), d4)    # run after run
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fs, ds = ED.eval_flow_records(fset, fp[:4]), ED.eval_depth_records(dset, dp[:4])
    side.synchronize()
    assert same(fs, f4) and same(ds, d4)
    assert bool(torch.isfinite(f4[:, :13]).all()) and bool(torch.isfinite(d4).all())


# ---------------------------------------------------------------------------------------------------------------- 5: bounds
def test_guarded_buffers_and_nan_padding():
    lib = get_lib()
    pred_hw = EC.PRED_SIZES[0]
    gts, nocs, movs, preds = EC.flow_case(pred_hw)
    gd, dd = EC.depth_case(pred_hw, "uniform")
    fset, dset = ED.FlowEvalSet(gts, nocs, movs, device=dev()), ED.DepthEvalSet(gd, device=dev())
    fp, dp = _flow_pred(preds), _disp(dd)
    n = 4
    clean_f, clean_d = ED.eval_flow_records(fset, fp[:n]), ED.eval_depth_records(dset, dp[:n])
    inputs = [fset.u, fset.v, fset.flags, fset.dims, dset.gt, dset.dims, fp, dp]
    before = [t.clone() for t in inputs]
    for rec_doubles, ws_bytes, run in ((16, lib.dfe_eval_flow_ws_bytes(n), lambda r, w: ED.eval_flow_records(fset, fp[:n], 0, r, w)),
                                       (10, lib.dfe_eval_depth_ws_bytes(n, dset.hmax, dset.wmax),
                                        lambda r, w: ED.eval_depth_records(dset, dp[:n], 0, r, w))):
        rec = G.Carved((n, 2 * rec_doubles))
        ws = G.CarvedBytes((ws_bytes,))
        assert ws_bytes > 0 and ws.ptr % 16 == 0
        run(rec.view, ws.view)
        torch.cuda.synchronize()
        assert rec.intact() and ws.intact()
        got = rec.view.view(torch.float64)
        assert torch.equal(got.view(torch.int64), (clean_f if rec_doubles == 16 else clean_d).view(torch.int64))
    assert all(torch.equal(a, b) for a, b in zip(inputs, before))                                 # the inputs are untouched
    # NaN in everything a kernel must not use: the planes' padding beyond H_i x W_i, and the workspace before the call (its
    # pred planes keep the NaN wherever the mask is off)
    for i, (H, W) in enumerate(EC.GT_SIZES):
        for plane in (fset.u, fset.v, dset.gt):
            plane[i, H:, :] = float("nan")
            plane[i, :, W:] = float("nan")
        fset.flags[i, H:, :] = 0xFF
        fset.flags[i, :, W:] = 0xFF
    ws_f = torch.full((lib.dfe_eval_flow_ws_bytes(n) // 4,), float("nan"), device=dev())
    ws_d = torch.full((lib.dfe_eval_depth_ws_bytes(n, dset.hmax, dset.wmax) // 4,), float("nan"), device=dev())
    nan_f, nan_d = ED.eval_flow_records(fset, fp[:n], 0, None, ws_f), ED.eval_depth_records(dset, dp[:n], 0, None, ws_d)
    assert torch.equal(nan_f.view(torch.int64), clean_f.view(torch.int64))
    assert torch.equal(nan_d.view(torch.int64), clean_d.view(torch.int64))
    planes = ws_d[:n * dset.hmax * dset.wmax].view(n, dset.hmax, dset.wmax).cpu().numpy()
    for i in range(n):
        m = np.zeros((dset.hmax, dset.wmax), bool)
        m[:gd[i].shape[0], :gd[i].shape[1]] = EC.depth_near(gd[i], dd[i])[1]
        assert np.isfinite(planes[i][m]).all() and np.isnan(planes[i][~m]).all()                 # pred written under the mask alone


# ---------------------------------------------------------------------------------------------------------------- 6: Evaluator
@pytest.fixture
def deterministic():
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)       # the nets' outputs repeat bit for bit: what passes once passes always
    yield
    convs.set_deterministic(before)


def _values(table):
    return [float(v) for v in str(table).strip().split("\n")[1].split(",")]


def test_evaluator_against_the_per_image_path(tmp_path):
    """Seed 0 of Model_geometry; no other seed was needed (a decision of a random net's prediction inside the rounding of a
    threshold would move a1-a3 or the outlier rates by 1 / count, far above the tolerances)."""
    drv = _driver("test")
    cfg = EC.mini_tree(str(tmp_path))
    torch.manual_seed(0)
    model = get_model("geom")(make_cfg(num_scales=3, img_hw=cfg.img_hw, mode="geom")).to(dev())
    model.train()
    list(model.modules())[-1].eval()                      # one module in another mode: restored as it was, not as its parent
    state = {k: v.clone() for k, v in model.state_dict().items()}
    modes = [m.training for m in model.modules()]
    ev = ED.Evaluator(model, cfg, flow_2012=ED.FlowEvalSet.from_kitti(cfg.gt_2012_dir, cfg.img_hw, 2012, dev()),
                      flow_2015=ED.FlowEvalSet.from_kitti(cfg.gt_2015_dir, cfg.img_hw, 2015, dev()),
                      depth=ED.DepthEvalSet.from_eigen(cfg.raw_base_dir, cfg.eigen_dir, cfg.img_hw, dev()), batch=2)
    out = ev.run()
    assert [m.training for m in model.modules()] == modes
    again = ev.run()                                      # a second run on the same session: same tables (MIOpen repeats to rounding)
    assert [m.training for m in model.modules()] == modes and ev._session.stats()["folds"] == 2      # invalidated every time
    np.testing.assert_allclose(_values(again["eval_2015_res"]), _values(out["eval_2015_res"]), **FLOW_TOL)
    np.testing.assert_allclose(again["eval_eigen_res"], out["eval_eigen_res"], **DEPTH_TOL)
    after = model.state_dict()
    assert list(after) == list(state)
    for k, v in state.items():                            # num_batches_tracked and the running statistics included
        assert v.dtype == after[k].dtype and torch.equal(v.view(torch.uint8) if v.dim() else v, after[k].view(torch.uint8) if v.dim() else after[k]), k
    model.eval()
    ref12, ref15 = drv.test_kitti_flow(cfg, model, dev(), 2012), drv.test_kitti_flow(cfg, model, dev(), 2015)
    refd = drv.test_eigen_depth(cfg, model, dev())
    print("\n2012 fused  %s\n2012 image  %s\n2015 fused  %s\n2015 image  %s\ndepth fused %s\ndepth image %s"
          % (_values(out["eval_2012_res"]), _values(ref12), _values(out["eval_2015_res"]), _values(ref15), out["eval_eigen_res"], refd))
    assert out["eval_2012_res"].split("\n")[0] == ref12.split("\n")[0] and out["eval_2015_res"].split("\n")[0] == ref15.split("\n")[0]
    assert len(_values(ref12)) == 4 and len(_values(ref15)) == 8
    np.testing.assert_allclose(_values(out["eval_2012_res"]), _values(ref12), **FLOW_TOL)
    np.testing.assert_allclose(_values(out["eval_2015_res"]), _values(ref15), **FLOW_TOL)
    np.testing.assert_allclose(out["eval_eigen_res"], refd, **DEPTH_TOL)
    # test.py --fused_eval: the same sets and Evaluator behind the tasks' own print-out
    np.testing.assert_allclose(drv.test_fused(cfg, model, dev(), "kitti_depth"), refd, **DEPTH_TOL)
    np.testing.assert_allclose(_values(drv.test_fused(cfg, model, dev(), "kitti_flow_2015")), _values(ref15), **FLOW_TOL)


# ---------------------------------------------------------------------------------------------------------------- training
def _flow_model_and_set(hw=(64, 128)):
    cfg = make_cfg(num_scales=3, img_hw=hw, mode="flow")
    torch.manual_seed(0)
    model = get_model("flow")(cfg).to(dev()).train()
    gts, nocs, movs, _ = EC.flow_case((16, 32), sizes=EC.GT_SIZES[:3])
    gen = torch.Generator().manual_seed(5)
    pairs = torch.rand((3, 3, 2 * hw[0], hw[1]), generator=gen)
    return cfg, model, gts, nocs, movs, pairs


def test_an_evaluation_between_two_steps_changes_nothing(deterministic):
    """Model_flow, B = 1, deterministic mode, FusedAdam.  At 128 x 128, not 64 x 128: the deterministic mode refuses the context
    network's dilation-16 layer on a quarter-size plane of fewer than 32 rows (its phase images would have one row), so 128 rows
    are the fewest a deterministic step of this model runs at."""
    hw = (128, 128)

    def two_steps(evaluate):
        cfg, model, gts, nocs, movs, pairs = _flow_model_and_set(hw)
        opt = make_optimizer(model, 1e-4)
        assert type(opt).__name__ == "FusedAdam"
        ev = ED.Evaluator(model, cfg, flow_2015=ED.FlowEvalSet(gts, nocs, movs, pairs, dev()), batch=2)
        got = {}
        for step in range(2):
            inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, hw[0], hw[1], 3, seed=10 + step)]
            loss, pack, _ = train_step(model, opt, inputs, cfg)
            got["loss%d" % step] = loss.detach().clone().reshape(-1).float()
            for k, v in pack.items():
                got["%s.%d" % (k, step)] = v.detach().clone().reshape(-1).float()
            if step == 0 and evaluate:
                res = ev.run()
                assert model.training and "err_rate" in res["eval_2015_res"]
        for name, p in model.named_parameters():
            got["p." + name] = p.detach().clone().reshape(-1)
            if p.grad is not None:
                got["g." + name] = p.grad.detach().clone().reshape(-1)
        return got
    a, b = two_steps(False), two_steps(True)
    assert list(a) == list(b) and any(k.startswith("g.") for k in a)
    bad = [k for k in a if not G.bits_equal(a[k], b[k])]
    assert bad == [], bad[:5]


def test_graph_session_gives_the_eager_tables():
    """session="graph": every batch shape (two and the tail of one) replays a captured call; same tables to the tolerance of test 1
    (MIOpen's convolutions repeat to rounding only)."""
    cfg, model, gts, nocs, movs, pairs = _flow_model_and_set()
    fset = ED.FlowEvalSet(gts, nocs, movs, pairs, dev())
    eager = ED.Evaluator(model, cfg, flow_2015=fset, batch=2).run()
    ev = ED.Evaluator(model, cfg, flow_2015=fset, batch=2, session="graph")
    graph = ev.run()
    assert ev._session.stats()["captures"] == 2 and ev._session.stats()["replays"] == 2 and model.training
    np.testing.assert_allclose(_values(graph["eval_2015_res"]), _values(eager["eval_2015_res"]), **FLOW_TOL)
    with pytest.raises(ValueError):
        ED.Evaluator(model, cfg, flow_2015=fset, session="off")
    with pytest.raises(ValueError, match="infer_depth"):
        ED.Evaluator(model, cfg, depth=ED.DepthEvalSet([np.full((37, 61), 5.0, np.float32)], torch.rand(1, 3, 64, 128), dev()))


def test_periodic_eval_prints_the_tables_and_grows_log_pkl(tmp_path, capsys):
    T = _driver("train")
    cfg, model, gts, nocs, movs, pairs = _flow_model_and_set()
    cfg.test_interval, cfg.no_test, cfg.model_dir = 1, False, str(tmp_path)
    ev = ED.Evaluator(model, cfg, flow_2012=ED.FlowEvalSet(gts, nocs, None, pairs, dev()),
                      flow_2015=ED.FlowEvalSet(gts, nocs, movs, pairs, dev()), batch=2)
    logs = []
    for it in range(2):
        pack = T.periodic_eval(cfg, ev, it, logs)
        assert sorted(pack) == ["eval_2012_res", "eval_2015_res"] and model.training
        with open(os.path.join(str(tmp_path), "log.pkl"), "rb") as fh:
            stored = pickle.load(fh)
        assert isinstance(stored, list) and len(stored) == it + 1 and stored[-1] == pack and all(isinstance(p, dict) for p in stored)
    text = capsys.readouterr().out
    assert text.count("[EVAL] [KITTI 2012]") == 2 and text.count("[EVAL] [KITTI 2015]") == 2
    assert "epe_noc" in text and "move_err_rate" in text
    assert text.index("[EVAL] [KITTI 2012]") < text.index("[EVAL] [KITTI 2015]")
