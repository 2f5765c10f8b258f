#!/usr/bin/env python3
"""Training driver with the reference's CLI surface (train.py:227-250) on the MI355X engine.

  python train.py -c config/kitti_geom.yaml --mode geom --model_dir ./models --batch_size 4
  torchrun --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 train.py -c config/kitti_geom.yaml --mode geom

Differences from the reference, all forced by what it cannot do: data parallelism is one process per GPU
with one process per GPU over RCCL (ddp.wrap: one flat gradient all-reduce per step) instead of nn.DataParallel (``--multi_gpu`` is accepted and ignored; launch with
torchrun); the data source is the synthetic KITTI-shaped triplet generator by default (``data_source: synthetic``), or the
reference's prepared KITTI tree with ``--data_source prepared --prepared_base_dir DIR`` (train.txt, stacked-triplet PNGs and
calib files as KITTI_RAW.prepare_data_mp writes them; read by prepared_data.PreparedFeeder on ``--num_workers`` decode threads
with the image half on the device), or the same tree kept in device memory with ``--data_source resident`` (prepared_data.ResidentTrainSet:
every distinct frame resized once, a batch is one gather launch; ``--resident_cache DIR`` keeps the built set on disk).  Periodic KITTI evaluation (train.py:136-164) is honoured: every ``--test_interval``
iterations (iteration 0 included) unless ``--no_test``, rank 0 runs KITTI flow 2012 / 2015 and / or Eigen depth by mode
(``periodic_eval``) from device-resident sets (eval_device.Evaluator: batched inference through an InferenceSession, metric
kernels behind each batch, one host transfer per task), prints the reference's tables and pickles the list of result packs to
``model_dir/log.pkl`` (the format of the reference's Visualizer.dump_log).  A task runs when the config names its data and the
directory exists (``gt_2012_dir``, ``gt_2015_dir``, ``raw_base_dir`` + ``eigen_dir``); the shipped config names none, so with it
nothing is evaluated.
Checkpoints keep the reference format: {iteration, model_state_dict, optimizer_state_dict} in
iter_{N}.pth and last.pth (train.py:21-29)."""
import argparse
import os
import pickle
import shutil
import time

import torch
import yaml

from unsupervised_depth_opticalflow_egomotion_amd import convs, ddp, ops, prepared_data, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import train_step, make_optimizer, GraphedTrainStep, LOSS_WEIGHT_ATTR


class pObject(object):
    pass


def save_model(iter_, model_dir, filename, model, optimizer):
    torch.save({"iteration": iter_, "model_state_dict": ddp.unwrap(model).state_dict(),
                "optimizer_state_dict": optimizer.state_dict()}, os.path.join(model_dir, filename))


def load_model(model_dir, filename, model, optimizer):
    data = torch.load(os.path.join(model_dir, filename), map_location="cpu")
    ddp.unwrap(model).load_state_dict(data["model_state_dict"])
    optimizer.load_state_dict(data["optimizer_state_dict"])
    return data["iteration"], model, optimizer


def print_loss(iter_, loss_pack, weights, total, guard=None):
    """``guard``: FusedAdam.guard_stats() when the gradient guard is on (--clip_grad_norm / --skip_nonfinite)."""
    line = "iter {:6d} total {:.4f} | ".format(iter_, float(total))
    line += " ".join("{}:{:.4f}".format(k.replace("loss_", ""), float(v.mean()) * weights[k]) for k, v in loss_pack.items())
    if guard is not None:
        line += " | gnorm {:.2f} clip {:.2f} skipped {:d}".format(guard["grad_norm"], guard["clip_coef"], guard["skipped_steps"])
    print(line, flush=True)


def build_evaluator(cfg, model, dev):
    """The evaluator of the mode's tasks whose data the config names and which exist (None: nothing to evaluate).  The sets are read
    and prepared here, once."""
    from unsupervised_depth_opticalflow_egomotion_amd import eval_device
    if getattr(cfg, "no_test", False):
        return None
    sets = {}
    for task in eval_device.tasks_for_mode(cfg.mode):
        if task == "depth":
            raw, eigen = getattr(cfg, "raw_base_dir", None), getattr(cfg, "eigen_dir", None)
            if raw and eigen and os.path.isdir(raw) and os.path.isdir(eigen):
                sets[task] = eval_device.DepthEvalSet.from_eigen(raw, eigen, cfg.img_hw, dev)
        else:
            year = int(task[-4:])
            gt_dir = getattr(cfg, "gt_%d_dir" % year, None)
            if gt_dir and os.path.isdir(gt_dir):
                sets[task] = eval_device.FlowEvalSet.from_kitti(gt_dir, cfg.img_hw, year, dev)
    if not sets:
        return None
    return eval_device.Evaluator(ddp.unwrap(model), cfg, **sets)


def periodic_eval(cfg, evaluator, it, log_list):
    """train.py:136-164: at ``it % test_interval == 0`` unless ``no_test``, run the evaluator, print the reference's lines, append
    the result pack to ``log_list`` and pickle the list to ``model_dir/log.pkl``.  Returns the pack, or None when nothing ran."""
    if evaluator is None or getattr(cfg, "no_test", False) or it % cfg.test_interval != 0:
        return None
    pack = evaluator.run()
    for year in (2012, 2015):
        if "eval_%d_res" % year in pack:
            print("[EVAL] [KITTI %d]" % year)
            print(pack["eval_%d_res" % year], flush=True)
    if "eval_eigen_res" in pack:
        print("[EVAL] [KITTI Eigen depth]")
        print("{:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10} ".format("abs_rel", "sq_rel", "rms", "log_rms", "a1", "a2", "a3"))
        print("{:10.4f}, {:10.4f}, {:10.3f}, {:10.3f}, {:10.3f}, {:10.3f}, {:10.3f} ".format(*pack["eval_eigen_res"]), flush=True)
    log_list.append(pack)
    with open(os.path.join(cfg.model_dir, "log.pkl"), "wb") as fh:
        pickle.dump(log_list, fh)
    return pack


def train(cfg):
    world, rank, local = ddp.init_process_group()
    dev = torch.device("cuda", local) if torch.cuda.is_available() else None
    if dev is None:
        raise RuntimeError("train.py needs a HIP device: the loss stack has no CPU fallback")
    ops.set_align_corners(bool(getattr(cfg, "align_corners", False)))
    # --deterministic / the YAML key switch the mode on; they never switch off what DFE_DETERMINISTIC=1 asked for
    convs.set_deterministic(convs.DETERMINISTIC or bool(getattr(cfg, "deterministic", False)))
    if convs.DETERMINISTIC:      # the step is a pure function of weights and inputs: the initial weights come from a seed too (YAML 'seed')
        torch.manual_seed(int(getattr(cfg, "seed", 0)))
    model = get_model(cfg.mode)(cfg)
    if cfg.mode == "geom":
        for attr, path in (("flow_pretrained_model", ("fpyramid.", "pwc_model.")),
                           ("depth_pretrained_model", ("depth_net.", "pose_net."))):
            f = getattr(cfg, attr, None)
            if f:
                data = torch.load(f, map_location="cpu")["model_state_dict"]
                data = {k.replace("module.", "", 1): v for k, v in data.items()}
                print("load %s from %s" % (attr, f))
                model.load_state_dict({k: v for k, v in data.items() if k.startswith(path)}, strict=False)
    model = model.to(dev)
    for flag, names in (("fix_depth", ("depth_net",)), ("fix_pose", ("pose_net",)), ("fix_flow", ("fpyramid", "pwc_model"))):
        if getattr(cfg, flag, False):
            for name, p in model.named_parameters():
                if any(n in name for n in names):
                    p.requires_grad = False
    model.train()
    model = ddp.wrap(model, dev)
    use_graph = bool(getattr(cfg, "graph", False)) and world == 1
    # 0 / absent: off (then DFE_CLIP_GRAD_NORM / DFE_SKIP_NONFINITE decide, see make_optimizer)
    optimizer = make_optimizer(model, cfg.lr, capturable=use_graph, max_grad_norm=float(getattr(cfg, "clip_grad_norm", 0) or 0) or None,
                               skip_nonfinite=bool(getattr(cfg, "skip_nonfinite", False)))
    guarded = getattr(optimizer, "max_grad_norm", None) is not None or getattr(optimizer, "skip_nonfinite", False)
    start = 0
    if cfg.resume:
        fn = "iter_{}.pth".format(cfg.iter_start) if cfg.iter_start > 0 else "last.pth"
        start, model, optimizer = load_model(cfg.model_dir, fn, model, optimizer)
    weights = {k: getattr(cfg, a) for k, a in LOSS_WEIGHT_ATTR.items()}
    h, w = cfg.img_hw
    n_iter = cfg.num_iterations - start
    raw_pipeline = bool(getattr(cfg, "device_pipeline", False))
    feeder, train_set = None, None
    if getattr(cfg, "data_source", "synthetic") == "prepared":     # the reference's prepared tree (train.py:100-125)
        if not getattr(cfg, "prepared_base_dir", None):
            raise ValueError("data_source 'prepared' needs prepared_base_dir (--prepared_base_dir or the YAML key)")
        source = prepared_data.PreparedKITTI(cfg.prepared_base_dir, cfg.num_scales, (h, w))
        feeder = prepared_data.PreparedFeeder(source, cfg.batch_size, (h, w), dev, n_iter, num_workers=cfg.num_workers,
                                              world=world, rank=rank)
        if rank == 0:
            print("A total of {} image pairs found".format(source.count()), flush=True)
    elif getattr(cfg, "data_source", "synthetic") == "resident":   # the same tree, resident in HBM: no decode, no copy per step
        if not getattr(cfg, "prepared_base_dir", None):
            raise ValueError("data_source 'resident' needs prepared_base_dir (--prepared_base_dir or the YAML key)")
        source = prepared_data.PreparedKITTI(cfg.prepared_base_dir, cfg.num_scales, (h, w))
        reserve = getattr(cfg, "resident_reserve_mb", None)
        train_set = prepared_data.ResidentTrainSet(source, (h, w), dev, num_workers=cfg.num_workers,
                                                   cache_dir=getattr(cfg, "resident_cache", None), write_cache=rank == 0,
                                                   reserve_mb=prepared_data.RESIDENT_RESERVE_MB if reserve is None else reserve)
        feeder = train_set.batches(cfg.batch_size, n_iter, world=world, rank=rank)      # every rank holds the whole set
        if rank == 0:
            print("A total of {} image pairs found".format(source.count()), flush=True)
            print("resident set: {} frames, {} bytes, {} in {:.1f} s".format(
                train_set.F, train_set.nbytes, "loaded from the cache" if train_set.from_cache else "built", train_set.build_seconds),
                flush=True)
    elif raw_pipeline:   # raw uint8 triplets at KITTI's native size; resize / flip / normalise run on the device
        dataset = synthetic.SyntheticRawTriplets(n_iter * cfg.batch_size * world, (375, 1242), (h, w), cfg.num_scales, seed=1234)
    else:
        dataset = synthetic.SyntheticTriplets(n_iter * cfg.batch_size * world, (h, w), cfg.num_scales, seed=1234)
    prof, graphed = None, None
    if getattr(cfg, "profile", False):       # the reference's Profiler marks (core/visualize/profiler.py) + roctx ranges per HIP launcher
        from unsupervised_depth_opticalflow_egomotion_amd import profiling
        profiling.enable()
        prof = profiling.Profiler(silent=rank != 0)
    evaluator, log_list = (build_evaluator(cfg, model, dev) if rank == 0 else None), []      # rank 0 alone evaluates; no collective
    t0 = time.time()
    for it in range(start, cfg.num_iterations):
        periodic_eval(cfg, evaluator, it, log_list)
        if train_set is not None and graphed is not None:
            # The gather runs OUTSIDE the captured graph (its arguments -- the batch's triplets and flips -- change per step) and
            # writes straight into the graph's static inputs; graphed(...) then sees equal pointers and copies nothing.
            inputs = train_set.fetch(it - start, out=graphed.static_inputs)
        elif feeder is not None:
            inputs = next(feeder)      # batch it - start of the per-rank shard: idx = (it - start) * B * world + rank * B + j
        else:
            base = (it - start) * cfg.batch_size * world + rank * cfg.batch_size
            samples = [dataset[base + j] for j in range(cfg.batch_size)]
            if raw_pipeline:
                raw = torch.stack([s[0] for s in samples]).pin_memory().to(dev, non_blocking=True)
                flip = torch.tensor([s[3] for s in samples], dtype=torch.uint8)
                inputs = [ops.prepare_triplets(raw, (h, w), flip)] + \
                    [torch.stack([s[i] for s in samples]).to(dev, non_blocking=True) for i in (1, 2)]
            else:
                inputs = [torch.stack([s[i] for s in samples]).to(dev, non_blocking=True) for i in range(3)]
        if prof is not None:
            prof.reset()
        if use_graph:      # one hipGraph launch per iteration (train_step.GraphedTrainStep): captured on the first batch
            if graphed is None:
                graphed = GraphedTrainStep(model, optimizer, inputs, cfg)
            loss, loss_pack, mask_pack = graphed(inputs)
        else:
            loss, loss_pack, mask_pack = train_step(model, optimizer, inputs, cfg, prof if (prof is not None and it % cfg.log_interval == 0) else None)
        if rank == 0 and it % cfg.log_interval == 0:
            print_loss(it, loss_pack, weights, loss, optimizer.guard_stats() if guarded else None)
        if rank == 0 and (it + 1) % cfg.save_interval == 0:
            save_model(it + 1, cfg.model_dir, "iter_{}.pth".format(it + 1), model, optimizer)
            save_model(it + 1, cfg.model_dir, "last.pth", model, optimizer)
    if feeder is not None:
        feeder.close()
    if rank == 0:
        print("done: %d iterations in %.1f s" % (cfg.num_iterations - start, time.time() - t0))
    if world > 1:
        torch.distributed.destroy_process_group()


# CLI attributes that leave the YAML's value alone when they are not given
KEEP_YAML_WHEN_UNSET = ("num_iterations", "data_source", "prepared_base_dir", "resident_cache", "deterministic", "clip_grad_norm", "skip_nonfinite")


def build_parser():
    ap = argparse.ArgumentParser(description="joint depth / flow / pose training on MI355X")
    ap.add_argument("-c", "--config_file", default="config/kitti_geom.yaml")
    ap.add_argument("-g", "--gpu", type=str, default="0", help="kept for CLI compatibility; use torchrun for >1 GPU")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--iter_start", type=int, default=0)
    ap.add_argument("--lr", type=float, default=0.0001)
    ap.add_argument("--num_workers", type=int, default=6)
    ap.add_argument("--log_interval", type=int, default=100)
    ap.add_argument("--test_interval", type=int, default=2000)
    ap.add_argument("--save_interval", type=int, default=2000)
    ap.add_argument("--vis_interval", type=int, default=100)
    ap.add_argument("--mode", type=str, default="geom", help="flow | depth | geom")
    ap.add_argument("--model_dir", type=str, default=None)
    ap.add_argument("--prepared_save_dir", type=str, default="data_s1")
    ap.add_argument("--data_source", type=str, default=None, choices=("synthetic", "prepared", "resident"),
                    help="synthetic triplets (the YAML's default), the reference's prepared KITTI tree under --prepared_base_dir "
                         "streamed from the host, or ('resident') the same tree kept in device memory: every rank holds the whole set")
    ap.add_argument("--prepared_base_dir", type=str, default=None,
                    help="directory holding train.txt, the stacked-triplet PNGs and calib files (KITTI_RAW.prepare_data_mp's output)")
    ap.add_argument("--resident_cache", type=str, default=None,
                    help="with --data_source resident: a directory that keeps the built set (frames.u8, tri.i32, K.f32, meta.json); "
                         "loaded instead of decoding when its key matches the tree (also the YAML key 'resident_cache'; the reserve "
                         "left for the step is the YAML key 'resident_reserve_mb')")
    ap.add_argument("--flow_pretrained_model", type=str, default=None)
    ap.add_argument("--depth_pretrained_model", type=str, default=None)
    ap.add_argument("--resume", action="store_true")
    ap.add_argument("--multi_gpu", action="store_true")
    ap.add_argument("--no_test", action="store_true")
    ap.add_argument("--fix_depth", action="store_true")
    ap.add_argument("--fix_pose", action="store_true")
    ap.add_argument("--fix_flow", action="store_true")
    ap.add_argument("--num_iterations", type=int, default=None)
    ap.add_argument("--graph", action="store_true",
                    help="capture the whole training step (three network streams, loss stack, backward, Adam) in a hipGraph after three "
                         "eager steps and replay it: one launch per iteration (single process, static shapes; pays when the host is the "
                         "bound, e.g. small batches)")
    ap.add_argument("--profile", action="store_true",
                    help="roctx ranges around every HIP launcher (rocprofv3 --marker-trace) and the reference Profiler's forward / backward / "
                         "optimizer wall times at every log interval (synchronises the device at each mark)")
    ap.add_argument("--deterministic", action="store_const", const=True, default=None,
                    help="no convolution of the step reaches MIOpen: every pass on this build's fixed-order kernels, so that loss, outputs "
                         "and gradients repeat bit for bit run after run and process after process (same build, GPU model, batch and "
                         "inputs; slower; also the YAML key 'deterministic' and DFE_DETERMINISTIC=1)")
    ap.add_argument("--device_pipeline", action="store_true",
                    help="feed raw uint8 triplets and run resize / flip / normalise on the device (ops.prepare_triplets)")
    ap.add_argument("--clip_grad_norm", type=float, default=None,
                    help="clip the global 2-norm of the gradients to this value inside the optimiser step "
                         "(torch.nn.utils.clip_grad_norm_'s formula, on the device; also the YAML key 'clip_grad_norm' and "
                         "DFE_CLIP_GRAD_NORM; 0: off)")
    ap.add_argument("--skip_nonfinite", action="store_const", const=True, default=None,
                    help="do not apply a step whose gradients hold a NaN or an inf: parameters, moments and Adam's step count stay "
                         "as they are and the skip is counted (also the YAML key 'skip_nonfinite' and DFE_SKIP_NONFINITE=1)")
    return ap


def merge_cfg(args, cfg):
    """The YAML's dict with the command line on top: every CLI attribute overrides / extends it (train.py:272-274), except
    the ones of KEEP_YAML_WHEN_UNSET when they were not given."""
    cfg = dict(cfg)
    cfg["img_hw"] = (cfg["img_hw"][0], cfg["img_hw"][1])
    cfg["model_dir"] = os.path.join(args.model_dir or "./models", args.mode)
    for k, v in vars(args).items():
        if k in ("model_dir",) or (k in KEEP_YAML_WHEN_UNSET and v is None):
            continue
        cfg[k] = v
    return cfg


if __name__ == "__main__":
    args = build_parser().parse_args()
    with open(args.config_file) as fh:
        cfg = merge_cfg(args, yaml.safe_load(fh))
    os.makedirs(cfg["model_dir"], exist_ok=True)
    if int(os.environ.get("RANK", "0")) == 0:
        shutil.copy(args.config_file, cfg["model_dir"])
        with open(os.path.join(cfg["model_dir"], "config.pkl"), "wb") as fh:
            pickle.dump(cfg, fh)
    cfg_new = pObject()
    for k, v in cfg.items():
        setattr(cfg_new, k, v)
    train(cfg_new)
