"""``python train.py config=unet config.key=value`` -- the reference's training entry point (train.py:90-388)
on the MI355X hot path: same config keys, registry names, init policy, optimizer / StepLR, step semantics
(train.py:187-221 via engine.train_step) and checkpoint format
(``{"model", "optim", "scheduler", "epoch"}`` in latest_checkpoint.pt / checkpoint_%04d.pt, train.py:285-306;
resume when load_mode == 1, train.py:123-140).  TensorBoard / rich / accelerate are replaced by a JSONL scalar
log, the logging module and mi355seg.distributed."""
import json
import logging
import os
import sys
import time

import torch
from torch.optim.lr_scheduler import StepLR

from . import distributed as D
from .config import absent as _absent, compose, parse_patch_size
from .data import make_loader
from . import functional as F
from .engine import GraphedTrainStep, _sync_metrics, make_adam, mixed_precision_dtype, train_step, weights_init_normal
from .registry import build_model
from .models.three_d.IS import set_band_split


LOSS_KEYS = ("loss_weights", "focal_gamma", "tversky_alpha", "tversky_beta", "cldice_weight", "cldice_iters", "cldice_smooth",
             "boundary_weight", "boundary_spacing", "boundary_ramp_epochs")


def parse_loss(config):
    """``config.loss`` -> the criterion of the run: None (the live BCE path of train.py:115, engine.train_step's default) when the key
    is absent, empty or "bce"; otherwise a utils.loss_function.CompoundLoss built from ``config.loss_weights=wv,wr``,
    ``config.focal_gamma``, ``config.tversky_alpha`` and ``config.tversky_beta`` (each only with a mode that has that term), and the
    soft-clDice term's ``config.cldice_weight`` (>= 0; 0 = no term), ``config.cldice_iters`` (1..32) and ``config.cldice_smooth``
    (> 0), which go with any compound mode, as do the boundary term's ``config.boundary_weight`` (>= 0; 0 = no term),
    ``config.boundary_spacing=sz,sy,sx`` (positive; default ``config.resample_spacing`` when that is set, else 1,1,1) and
    ``config.boundary_ramp_epochs`` (an integer >= 0, see ``boundary_ramp``; kept on the criterion as ``boundary_ramp_epochs``)."""
    from .utils.loss_function import CompoundLoss
    get = lambda k: config.get(k) if hasattr(config, "get") else getattr(config, k, None)
    mode = get("loss")
    allowed = ("bce",) + F.LOSS_MODES
    if not _absent(mode) and (not isinstance(mode, str) or mode not in allowed):
        raise ValueError(f"config.loss must be one of {', '.join(allowed)}, got {mode!r}")
    mode = None if _absent(mode) or mode == "bce" else mode
    given = {k: get(k) for k in LOSS_KEYS if not _absent(get(k))}
    has = {"loss_weights": mode is not None, "focal_gamma": mode in ("focal", "dice_focal"),
           "tversky_alpha": mode == "tversky", "tversky_beta": mode == "tversky"}
    compound = "a compound mode (" + ", ".join(F.LOSS_MODES) + ")"
    needs = {"loss_weights": compound, "focal_gamma": "focal or dice_focal", "tversky_alpha": "tversky", "tversky_beta": "tversky"}
    for k in ("cldice_weight", "cldice_iters", "cldice_smooth", "boundary_weight", "boundary_spacing", "boundary_ramp_epochs"):
        has[k], needs[k] = mode is not None, compound
    for k, v in given.items():
        if not has[k]:
            raise ValueError(f"config.{k} must be given only with config.loss = {needs[k]}, got {v!r} with config.loss={mode or 'bce'}")
    if mode is None:
        return None

    def number(k, rule, ok):
        v = given[k]
        if isinstance(v, str):
            try:
                v = float(v)
            except ValueError:
                v = None
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)):
            raise ValueError(f"config.{k} must be {rule}, got {given[k]!r}")
        return float(v)

    kw = {}
    if "loss_weights" in given:
        w = given["loss_weights"]
        parts = w.strip("()[] ").split(",") if isinstance(w, str) else (list(w) if hasattr(w, "__len__") else [w])
        bad = ValueError(f"config.loss_weights must be two numbers wv,wr (voxel term, region term), each >= 0, got {w!r}")
        try:
            vals = [float(p) for p in parts if not isinstance(p, bool)]
        except (TypeError, ValueError):
            raise bad from None
        if len(parts) != 2 or len(vals) != 2 or not all(v >= 0 for v in vals):
            raise bad
        kw["weights"] = tuple(vals)
    if "focal_gamma" in given:
        kw["focal_gamma"] = number("focal_gamma", "0 or a number in [1, 8]", lambda v: v == 0 or 1 <= v <= 8)
    for k in ("tversky_alpha", "tversky_beta"):
        if k in given:
            kw[k] = number(k, "a number >= 0", lambda v: v >= 0)
    if "cldice_weight" in given:
        kw["cldice_weight"] = number("cldice_weight", "a number >= 0", lambda v: v >= 0)
    if "cldice_smooth" in given:
        kw["cldice_smooth"] = number("cldice_smooth", "a number > 0", lambda v: v > 0)
    if "cldice_iters" in given:
        v = given["cldice_iters"]
        try:
            v = int(v) if isinstance(v, str) else v
        except ValueError:
            v = None
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= F.MAX_SKEL_ITERS:
            raise ValueError(f"config.cldice_iters must be an integer in 1..{F.MAX_SKEL_ITERS}, got {given['cldice_iters']!r}")
        kw["cldice_iters"] = v
    if "boundary_weight" in given:
        kw["boundary_weight"] = number("boundary_weight", "a number >= 0", lambda v: 0 <= v < float("inf"))
    spacing = given.get("boundary_spacing")
    if spacing is None and kw.get("boundary_weight", 0) > 0 and not _absent(get("resample_spacing")):
        from .resample import _parse_three
        spacing = _parse_three("resample_spacing", get("resample_spacing"))     # the grid the patches are drawn from
    if spacing is not None:
        parts = spacing.strip("()[] ").split(",") if isinstance(spacing, str) else (list(spacing) if hasattr(spacing, "__len__") else [spacing])
        bad = ValueError(f"config.boundary_spacing must be three positive numbers sz,sy,sx, got {spacing!r}")
        try:
            vals = [float(p) for p in parts if not isinstance(p, bool)]
        except (TypeError, ValueError):
            raise bad from None
        if len(parts) != 3 or len(vals) != 3 or not all(0 < v < float("inf") for v in vals):
            raise bad
        kw["boundary_spacing"] = tuple(vals)
    ramp = 0
    if "boundary_ramp_epochs" in given:
        v = given["boundary_ramp_epochs"]
        try:
            v = int(v) if isinstance(v, str) else v
        except ValueError:
            v = None
        if isinstance(v, bool) or not isinstance(v, int) or not v >= 0:
            raise ValueError(f"config.boundary_ramp_epochs must be an integer >= 0, got {given['boundary_ramp_epochs']!r}")
        ramp = v
    if mode == "tversky":
        a, b = kw.get("tversky_alpha", F.TVERSKY_ALPHA), kw.get("tversky_beta", F.TVERSKY_BETA)
        if not a + b > 0:
            raise ValueError(f"config.tversky_alpha and config.tversky_beta must not both be 0, got {a!r} and {b!r}")
    criterion = CompoundLoss(mode, **kw)
    criterion.boundary_ramp_epochs = ramp
    return criterion


def parse_multiclass(config, criterion, data_key="data_path"):
    """``config.multiclass`` -> K = ``config.out_classes`` when the key is true, None when it is absent or false (then nothing of the
    run changes).  The labels of the data set are the classes 0..K-1 (0 = background); the step takes the label path of
    engine.train_step.  Needs 2 <= out_classes <= 16, a compound ``config.loss`` (``criterion`` = what parse_loss
    returned; the fused label tail is the compound losses') and volumes: refused with ``<data_key>=synthetic``, whose labels are
    binary.  ``criterion`` = False skips the loss check (predict.py, where no loss runs)."""
    get = lambda k: config.get(k) if hasattr(config, "get") else getattr(config, k, None)
    v = get("multiclass")
    if _absent(v):
        return None
    if not isinstance(v, bool) and str(v).lower() not in ("true", "false", "1", "0", "yes", "no"):
        raise ValueError(f"config.multiclass must be true or false, got {v!r}")
    if str(v).lower() in ("false", "0", "no"):
        return None
    K = get("out_classes")
    if isinstance(K, bool) or not isinstance(K, int) or not 2 <= K <= F.MAX_LOSS_CLASSES:
        raise ValueError(f"config.multiclass needs config.out_classes in 2..{F.MAX_LOSS_CLASSES} (the labels 0..out_classes-1), got {K!r}")
    if criterion is None:
        raise ValueError("config.multiclass needs a compound config.loss (" + ", ".join(F.LOSS_MODES) + "): the BCE default has no label form")
    if str(get(data_key)) == "synthetic":
        raise ValueError(f"config.multiclass needs labelled volumes: {data_key}=synthetic draws binary labels")
    return K


def boundary_ramp(weight, epoch, ramp_epochs):
    """The factor of the boundary term during (1-based) ``epoch``: weight * min(1, epoch / ramp_epochs), the schedule of the paper
    (the term enters gradually); ramp_epochs = 0: always the weight."""
    return weight if ramp_epochs <= 0 else weight * min(1.0, epoch / ramp_epochs)


class AverageMeter:
    def __init__(self):
        self.val = self.sum = self.count = self.avg = 0.0

    def update(self, v, n=1):
        self.val = v
        self.sum += v * n
        self.count += n
        self.avg = self.sum / max(self.count, 1)


def get_logger(config):
    os.makedirs(config.hydra_path, exist_ok=True)
    log = logging.getLogger("mi355seg.train")
    log.setLevel(logging.DEBUG)
    log.handlers.clear()
    log.addHandler(logging.StreamHandler(sys.stdout))
    log.addHandler(logging.FileHandler(os.path.join(config.hydra_path, f"{config.job_name}.log")))
    log.propagate = False
    return log


def train(config, model, logger):
    rank, world, local = D.init_from_env()
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    model = model.to(device)
    # config.hip_graph=true: the iteration is captured once and replayed -- for launch-bound shapes (64^3 patches, UNETR's token
    # path); the learning rate then lives in a device tensor so that StepLR still reaches the captured step.  Data parallel: two
    # graphs (through backward, optimizer step) with the gradient reducer between their replays.
    # config.capturable_adam=true: the same device-resident optimizer state without the graph (eager runs that must match a graphed one)
    flag = lambda name: str(config.get(name) if hasattr(config, "get") else getattr(config, name, False)).lower() in ("1", "true", "yes")
    hip_graph = flag("hip_graph")
    optimizer = make_adam(model.parameters(), lr=torch.tensor(float(config.init_lr), device=device), capturable=True) if (hip_graph or flag("capturable_adam")) \
        else make_adam(model.parameters(), lr=config.init_lr)                   # train.py:109 (torch's fused single-kernel Adam on the GPU)
    scheduler = StepLR(optimizer, step_size=config.scheduler_step_size, gamma=config.scheduler_gamma) \
        if config.use_scheduler else None                                       # train.py:119-120
    elapsed_epochs = 0
    if config.load_mode == 1:                                                   # train.py:123-140
        logger.info(f"load model from: {config.ckpt}")
        ckpt = torch.load(config.ckpt, map_location="cpu")
        state = {k[len("module."):] if k.startswith("module.") else k: v for k, v in ckpt["model"].items()}
        model.load_state_dict(state)                                            # accepts the reference's DDP-prefixed keys
        optimizer.load_state_dict(ckpt["optim"])
        if scheduler is not None and ckpt.get("scheduler") is not None:
            scheduler.load_state_dict(ckpt["scheduler"])
        elapsed_epochs = ckpt["epoch"]
    model.train()
    scalars = open(os.path.join(config.hydra_path, "scalars.jsonl"), "a") if rank == 0 else None
    loader = make_loader(config, device, config.in_classes, seed=1234 + rank)
    # accelerator.prepare (train.py:167-169): rank 0's parameters / buffers everywhere (after the optional checkpoint
    # load, so a resumed rank 0 wins), flat buffers for the per-step broadcast, bucketed gradient reducer
    reducer = D.setup_replica(model)
    criterion = parse_loss(config)                                              # config.loss: None = the live BCE path (train.py:115)
    if criterion is not None:
        logger.info(f"loss: {criterion}")
    multiclass = parse_multiclass(config, criterion)                            # config.multiclass: K = out_classes, or None
    mc = {}
    if multiclass is not None:
        # the label-range counter: every step adds to it on the device, read once per epoch
        mc = {"multiclass": multiclass, "label_bad": torch.zeros(1, dtype=torch.int64, device=device)}
        logger.info(f"multi-class: labels 0..{multiclass - 1}, per-class Dice in scalars.jsonl")
    act_dtype = mixed_precision_dtype(config)                                   # Accelerator(mixed_precision=...) of train.py:167
    if act_dtype != torch.float32:
        logger.info(f"mixed precision: activations in {act_dtype} (fp32 parameters, gradients, statistics, loss)")
    epochs = config.epochs - elapsed_epochs
    graphed = None
    iteration = elapsed_epochs * len(loader)
    loss_meter, dice_meter = AverageMeter(), AverageMeter()
    for epoch in range(elapsed_epochs + 1, elapsed_epochs + epochs + 1):
        t_epoch = time.time()
        if criterion is not None and criterion.boundary_weight > 0:     # config.boundary_ramp_epochs; `epoch` survives a resume
            criterion.set_boundary_scale(boundary_ramp(criterion.boundary_weight, epoch, criterion.boundary_ramp_epochs))
        for i, batch in enumerate(loader):
            t0 = time.time()
            x, gt = batch["source"]["data"], batch["gt"]["data"]
            if world > 1:
                D.broadcast_buffers(model, async_op=True)               # launched here, waited for at the forward's first norm layer
            if hip_graph and graphed is None:
                # the first iteration runs inside the constructor (eager, on a side stream: workspaces sized, kernel attributes set),
                # then the iteration is captured for the following ones; a replay waits for the buffer broadcast launched above
                graphed = GraphedTrainStep(model, optimizer, x, gt, criterion=criterion, warmup=1, dtype=act_dtype, grad_hook=reducer,
                                           multiclass=multiclass)
                if multiclass is not None:
                    mc["label_bad"] = graphed.label_bad
                out = dict(graphed.first)
                _sync_metrics(out, multiclass)
            elif hip_graph:
                out = graphed(x, gt)
            else:
                out = train_step(model, optimizer, x, gt, criterion=criterion, grad_hook=reducer, dtype=act_dtype, **mc)    # train.py:187-221
            iteration += 1
            loss_meter.update(out["loss"].item(), x.size(0))
            dice_meter.update(out["dice"], x.size(0))
            if scalars:
                row = {"iteration": iteration, "Training/Loss": loss_meter.val, "Training/dice": dice_meter.val}
                if criterion is not None:                       # a compound loss: its terms, unweighted
                    for name, v in zip(criterion.term_names, out["loss_terms"].tolist()):
                        row[f"Training/loss_{name}"] = v        # voxel, region, then cldice / boundary when their weights are > 0
                if multiclass is not None:
                    for k in range(1, multiclass):
                        row[f"Training/dice_class_{k}"] = out["class_dice"][k]
                scalars.write(json.dumps(row) + "\n")
                scalars.flush()
            logger.info(f"\nEpoch: {epoch} Batch: {i}, train time: {time.time() - t0:.3f}s\nLoss: {loss_meter.val}\nDice: {dice_meter.val}\n")
        if multiclass is not None:
            bad = int(mc["label_bad"].item())                           # one D2H copy per epoch
            if bad:
                raise ValueError(f"config.multiclass: {bad} label voxels of epoch {epoch} are not integers in 0..{multiclass - 1} "
                                 f"(config.out_classes={multiclass})")
        if scheduler is not None:
            scheduler.step()
            logger.info(f"Learning rate:  {scheduler.get_last_lr()[0]}")
        logger.info(f"\nEpoch {epoch} used time:  {time.time() - t_epoch:.3f} s\nLoss Avg:  {loss_meter.avg}\nDice Avg:  {dice_meter.avg}\n")
        if rank == 0:
            state = {"model": model.state_dict(), "optim": optimizer.state_dict(),
                     "scheduler": scheduler.state_dict() if scheduler is not None else None, "epoch": epoch}
            torch.save(state, os.path.join(config.hydra_path, config.latest_checkpoint_file))
            if epoch % config.epochs_per_checkpoint == 0:
                torch.save(state, os.path.join(config.hydra_path, f"checkpoint_{epoch:04d}.pt"))
    if scalars:
        scalars.close()
    return {"loss_avg": loss_meter.avg, "dice_avg": dice_meter.avg, "epoch": elapsed_epochs + epochs}


def main(argv=None, conf_dir=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    conf_dir = conf_dir or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf")
    config = compose(conf_dir, argv, job_name="train")
    parse_patch_size(config)
    # ``accelerate launch --num_processes N train.py`` of the reference: ``config.gpus=N`` (or MI355SEG_GPUS=N) starts the N
    # ranks from here when no launcher did (WORLD_SIZE unset) -- before this process has made any GPU call -- and waits
    gpus = int(config.get("gpus", os.environ.get("MI355SEG_GPUS", 1)) or 1)
    if gpus > 1 and "WORLD_SIZE" not in os.environ:
        # always the repo-level wrapper (it puts the package on the path; this file uses relative imports and whatever
        # sys.argv[0] is -- pytest, ``python -c``, another driver script -- is not the train entry point)
        script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train.py")
        rc = D.self_launch(gpus, [script] + argv)
        if rc:
            raise SystemExit(rc)
        return config, None
    model = build_model(config)                          # train.py:324-373
    set_band_split(model, config)                        # config.band_split (IS only): fft | device
    model.apply(weights_init_normal(config.init_type))   # train.py:374
    logger = get_logger(config)
    logger.info("\nParameter Settings:\n" + "".join(f"{k}: {v}\n" for k, v in config.items()))
    result = train(config, model, logger)
    logger.info(f"scalar log saved in:{config.hydra_path}")
    return config, result


if __name__ == "__main__":
    main()
