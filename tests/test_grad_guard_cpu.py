"""CPU-only checks of the gradient guard's surface: make_optimizer refuses it where FusedAdam is not selected, FusedAdam
validates ``max_grad_norm``, train.py's parser and YAML merge carry the two keys, and the header declares the entry points
with the signatures the derived binding gives them."""
import argparse
import ctypes

import pytest
import torch

from unsupervised_depth_opticalflow_egomotion_amd import _lib
from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
from unsupervised_depth_opticalflow_egomotion_amd.train_step import guard_defaults, make_optimizer

P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture
def no_guard_env(monkeypatch):
    for k in ("DFE_CLIP_GRAD_NORM", "DFE_SKIP_NONFINITE", "DFE_FUSED_ADAM"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_make_optimizer_refuses_the_guard_on_cpu_parameters(no_guard_env):
    model = torch.nn.Linear(4, 3)
    assert isinstance(make_optimizer(model, 1e-3), torch.optim.Adam)
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(_lib.DfeError, match="FusedAdam.*HIP device"):
            make_optimizer(model, 1e-3, **kw)
    no_guard_env.setenv("DFE_FUSED_ADAM", "0")         # the reason named is still the first one that applies
    with pytest.raises(_lib.DfeError, match="FusedAdam"):
        make_optimizer(model, 1e-3, max_grad_norm=1.0)


def test_the_environment_sets_the_defaults(no_guard_env):
    assert guard_defaults() == (None, False)
    no_guard_env.setenv("DFE_CLIP_GRAD_NORM", "0")
    no_guard_env.setenv("DFE_SKIP_NONFINITE", "0")
    assert guard_defaults() == (None, False)
    assert isinstance(make_optimizer(torch.nn.Linear(2, 2), 1e-3), torch.optim.Adam)
    no_guard_env.setenv("DFE_CLIP_GRAD_NORM", "1e9")
    assert guard_defaults() == (1e9, False)
    with pytest.raises(_lib.DfeError, match="max_grad_norm"):
        make_optimizer(torch.nn.Linear(2, 2), 1e-3)
    no_guard_env.delenv("DFE_CLIP_GRAD_NORM")
    no_guard_env.setenv("DFE_SKIP_NONFINITE", "1")
    assert guard_defaults() == (None, True)
    with pytest.raises(_lib.DfeError, match="skip_nonfinite"):
        make_optimizer(torch.nn.Linear(2, 2), 1e-3)


@pytest.mark.parametrize("bad", [0, 0.0, -1, float("nan"), float("inf")])
def test_fused_adam_rejects_a_bad_max_grad_norm(bad):
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam([torch.nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


def test_the_guard_is_an_attribute_not_a_param_group_key():
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedAdam([p], max_grad_norm=2, skip_nonfinite=1)
    assert opt.max_grad_norm == 2.0 and isinstance(opt.max_grad_norm, float) and opt.skip_nonfinite is True
    off = FusedAdam([p])
    assert set(opt.param_groups[0]) == set(off.param_groups[0]) == set(opt.state_dict()["param_groups"][0])
    assert not any("norm" in k or "finite" in k for k in opt.param_groups[0])
    assert off.max_grad_norm is None and off.skip_nonfinite is False
    with pytest.raises(ValueError, match="guard_stats"):
        off.guard_stats()
    assert opt.guard_stats() == {"grad_norm": 0.0, "clip_coef": 1.0, "finite": True, "skipped_steps": 0}     # before the first step


def test_train_cli_and_yaml_merge():
    import train
    yaml_cfg = {"img_hw": [256, 832], "clip_grad_norm": 5.0, "skip_nonfinite": True, "deterministic": True}
    ap = train.build_parser()
    assert isinstance(ap, argparse.ArgumentParser)
    unset = train.merge_cfg(ap.parse_args([]), yaml_cfg)
    assert unset["clip_grad_norm"] == 5.0 and unset["skip_nonfinite"] is True and unset["deterministic"] is True
    assert unset["img_hw"] == (256, 832) and yaml_cfg["img_hw"] == [256, 832]
    given = train.merge_cfg(ap.parse_args(["--clip_grad_norm", "0.5", "--skip_nonfinite"]), {"img_hw": [256, 832], "skip_nonfinite": False})
    assert given["clip_grad_norm"] == 0.5 and given["skip_nonfinite"] is True
    absent = train.merge_cfg(ap.parse_args([]), {"img_hw": [256, 832]})
    assert "clip_grad_norm" not in absent and "skip_nonfinite" not in absent
    assert absent["batch_size"] == 8 and absent["graph"] is False           # every other attribute still lands in the cfg
    import os
    import yaml
    with open(os.path.join(os.path.dirname(os.path.abspath(train.__file__)), "config", "kitti_geom.yaml")) as fh:
        shipped = train.merge_cfg(ap.parse_args([]), yaml.safe_load(fh))
    assert not shipped.get("clip_grad_norm") and not shipped.get("skip_nonfinite")          # the shipped config leaves the guard off


def test_print_loss_line(capsys):
    import train
    pack = {"loss_flow_pixel": torch.tensor([2.0])}
    train.print_loss(7, pack, {"loss_flow_pixel": 0.5}, torch.tensor(1.0))
    plain = capsys.readouterr().out
    train.print_loss(7, pack, {"loss_flow_pixel": 0.5}, torch.tensor(1.0),
                     {"grad_norm": 12.344, "clip_coef": 0.8123, "finite": True, "skipped_steps": 3})
    assert capsys.readouterr().out == plain.rstrip("\n") + " | gnorm 12.34 clip 0.81 skipped 3\n"


SIGNATURES = {
    "dfe_grad_guard_ws_bytes": (I, [I]),
    "dfe_grad_guard_record_bytes": (I, []),
    "dfe_grad_guard": (I, [P, P, I, D, I, D, D, D, P, P, P, P, P]),
    "dfe_adam_tick_guarded": (I, [D, D, D, P, P, P, P]),
    "dfe_adam_step_guarded": (I, [P, P, I, D, D, D, P, P, P]),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_entry_points(name):
    restype, argtypes = SIGNATURES[name]
    assert _lib.header_signatures()[name] == (restype, argtypes)
    fn = getattr(_lib.get_lib(), name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes


def test_workspace_and_record_sizes_and_refusals_without_a_device():
    lib = _lib.get_lib()
    assert lib.dfe_grad_guard_record_bytes() == 32
    assert [lib.dfe_grad_guard_ws_bytes(n) for n in (-1, 0, 1, 7, 5400)] == [0, 0, 12, 84, 64800]
    # refused before any launch: no device is needed to be told so
    assert lib.dfe_grad_guard(None, None, 1, 1.0, 1, 1e-3, 0.9, 0.999, None, None, None, None, None) != 0
    assert lib.dfe_adam_step_guarded(None, None, 1, 0.9, 0.999, 1e-8, None, None, None) != 0
    assert lib.dfe_adam_tick_guarded(1e-3, 0.9, 0.999, None, None, None, None) != 0
