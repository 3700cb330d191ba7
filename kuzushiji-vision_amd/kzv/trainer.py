"""Training runtime standing in for the pieces of ``pl.Trainer`` the reference uses on this path
(scripts/train_trocr.py:165-176): one process per GPU, gradient all-reduce (mean) over RCCL overlapped with
backward, ``gradient_clip_val=1.0`` applied AFTER the reduce on the identical full gradient, optimizer step,
half-epoch validation, rank-0 logging/checkpoints.

DDP semantics reproduced: each rank's loss is the mean over ITS non-pad tokens; gradients are
summed across ranks and divided by world size; dropout streams differ per rank (seed mixes the rank).
"""
from __future__ import annotations

import ctypes as C
import os
import time

from . import _lib as L


def dist_env():
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    return rank, world, local


def dp_forced() -> bool:
    """Rehearsal switch: run the world > 1 code path (init_distributed, Stepper.step) with whatever world size there is."""
    return os.environ.get("KZV_FORCE_DIST", "0") not in ("", "0")


def init_distributed(backend: str | None = None):
    """torch.distributed over RCCL ("nccl" on ROCm) for GPUs, gloo on CPU.  No-op for world size 1 (unless KZV_FORCE_DIST)."""
    import torch
    import torch.distributed as dist
    rank, world, local = dist_env()
    # rehearsal knobs (1-GPU dev boxes): several ranks on one device over gloo
    if os.environ.get("KZV_FORCE_DEVICE") is not None:
        local = int(os.environ["KZV_FORCE_DEVICE"])
    backend = backend or os.environ.get("KZV_DIST_BACKEND")
    # KZV_FORCE_DIST=1: build the process group even for ONE rank, so that a 1-GPU box executes the data-parallel branch
    # end to end (RCCL communicator on the device, async all-reduce on RCCL's stream, CU reserve, segmented backward)
    if (world > 1 or dp_forced()) and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        if backend is None:
            backend = "nccl" if torch.cuda.is_available() else "gloo"
        if backend == "nccl":
            # RCCL's channel workgroups sit on CUs for the whole collective; keep them few (393 MB of gradients per
            # ~35 ms step needs little bandwidth) and tell the GEMM launchers to leave that many CUs alone, or the
            # one-workgroup-per-CU kernels would run a second round for the workgroups that found their CU taken
            os.environ.setdefault("NCCL_MAX_NCHANNELS", "16")
            if os.environ.get("KZV_CU_RESERVE") is None:
                L.check(L.load().kzv_set_cu_reserve(32), "set_cu_reserve")
            torch.cuda.set_device(local)
            dist.init_process_group(backend, rank=rank, world_size=world, device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world, local


def bucket_plan(seg_ranges, bucket_elems: int):
    """Merge consecutive backward segments (in completion order) into all-reduce buckets of at least
    ``bucket_elems`` fp32 elements.  Returns [(last_segment_index, lo, hi)] -- a bucket is launched once its
    last segment has been enqueued.  Ranges of merged segments are contiguous by construction of the
    parameter table (decoder at the tail, encoder layers in descending order, embeddings at the head)."""
    buckets = []
    cur_lo = cur_hi = None
    for i, (lo, hi) in enumerate(seg_ranges):
        if cur_lo is None:
            cur_lo, cur_hi = lo, hi
        else:
            if hi != cur_lo and lo != cur_hi:
                raise ValueError("segments are not contiguous in completion order")
            cur_lo, cur_hi = min(lo, cur_lo), max(hi, cur_hi)
        if cur_hi - cur_lo >= bucket_elems or i == len(seg_ranges) - 1:
            buckets.append((i, cur_lo, cur_hi))
            cur_lo = cur_hi = None
    return buckets


class Stepper:
    """One training step of the hot path: forward+loss, segmented backward with overlapped bucketed
    all-reduce, clip, RAdamScheduleFree step, bf16 weight refresh.

    ``accumulate_grad_batches = k > 1`` (Lightning's): ``step`` is then called once per micro-batch.  The gradient buffer is zeroed
    before a window's first micro-batch, every backward adds into it, the all-reduce runs only during the window's last backward
    (Lightning's no_sync) and ONE optimizer step closes the window with grad_scale = 1 / (k * world) -- also for the short window
    at the end of an epoch (``last_batch=True``), as Lightning divides every micro-batch loss by k.  ``stepped`` says whether the
    call ended in an optimizer step; the loss returned is then the mean of the window's micro-batch losses (summed on the device).
    With k = 1 (the default) a step launches exactly what it always launched."""

    def __init__(self, model, optimizer, world: int = 1, max_grad_norm: float = 1.0, bucket_mb: float = 64.0,
                 dp_path: bool | None = None, accumulate_grad_batches: int = 1):
        self.model, self.opt, self.world, self.max_grad_norm = model, optimizer, world, max_grad_norm
        # the data-parallel branch of step(); with one rank it is a rehearsal (a 1-rank all-reduce is the identity)
        self.dp_path = (world > 1 or dp_forced()) if dp_path is None else bool(dp_path)
        self._init_window(accumulate_grad_batches)
        lib = L.load()
        n = lib.kzv_backward_segments(model._h)
        # a frozen bottom of the encoder: the segments below the cut launch nothing, their ranges are never all-reduced
        frozen = lib.kzv_get_frozen_encoder_layers(model._h)
        if frozen > 0:
            n = n - 1 - frozen
        self.seg_ranges = []
        for s in range(n):
            lo, hi = C.c_int64(), C.c_int64()
            L.check(lib.kzv_backward_segment_range(model._h, s, C.byref(lo), C.byref(hi)), "segment_range")
            self.seg_ranges.append((lo.value, hi.value))
        # xGMI is point-to-point (7 links x ~153 GB/s): few large buckets keep every link busy and the launch
        # count low; 64 MB fp32 buckets -> ~7 collectives per 393 MB gradient set.
        self.buckets = bucket_plan(self.seg_ranges, int(bucket_mb * 1024 * 1024 / 4))

    def _init_window(self, k) -> None:
        if isinstance(k, bool) or int(k) != k or int(k) < 1:
            raise ValueError(f"accumulate_grad_batches must be an integer >= 1, not {k!r}")
        self.accumulate_grad_batches = int(k)
        self._micro = 0              # micro-batches of the open window that have run
        self._loss_sum = None        # their losses, added up on the device
        self.stepped = False

    # ---- the four device operations of a micro-batch (a test replaces them to record the schedule) ----
    def _forward(self, batch):
        loss, _ = self.model.forward_loss(batch["pixel_values"], batch["labels"], want_logits=False)
        return loss

    def _zero(self) -> None:
        L.check(L.load().kzv_zero_grads(self.model._h, L.stream_handle()), "zero_grads")

    def _backward(self, sync: bool) -> None:
        """The backward of the last forward, adding into the gradient buffer; ``sync``: all-reduce the buckets as their segments finish."""
        m, lib, st = self.model, L.load(), L.stream_handle()
        if not self.dp_path:     # no consumer between segments: let the engine overlap across them
            L.check(lib.kzv_backward(m._h, st), "backward")
            return
        if not sync:             # no_sync: the same segmented launches, no collective
            for s in range(len(self.seg_ranges)):
                L.check(lib.kzv_backward_segment(m._h, s, st), "backward_segment")
            return
        import torch.distributed as dist
        works = []
        bi = 0
        for s in range(len(self.seg_ranges)):
            L.check(lib.kzv_backward_segment(m._h, s, st), "backward_segment")
            if s == self.buckets[bi][0]:
                _, lo, hi = self.buckets[bi]
                # async: RCCL waits for the kernels enqueued so far on this stream, then runs on its own
                # stream while the remaining backward segments keep the compute stream busy
                works.append(dist.all_reduce(m.flat_grads[lo:hi], op=dist.ReduceOp.SUM, async_op=True))
                bi += 1
        for w in works:
            w.wait()

    def _opt_step(self, grad_scale: float) -> None:
        self.opt.step(max_grad_norm=self.max_grad_norm, grad_scale=grad_scale)

    def step(self, batch, batch_idx: int = 0, last_batch: bool = False):
        k = self.accumulate_grad_batches
        if k == 1:
            loss = self._forward(batch)
            self._zero()
            self._backward(True)
            self._opt_step(1.0 / self.world if self.dp_path else 1.0)
            self.stepped = True
            return loss
        loss = self._forward(batch)
        if self._micro == 0:
            self._zero()
            self._loss_sum = loss.clone()
        else:
            self._loss_sum += loss           # _loss is one device scalar overwritten per forward
        self._micro += 1
        closing = self._micro == k or last_batch
        self._backward(closing)
        self.stepped = closing
        if not closing:
            return None
        self._opt_step(1.0 / (k * self.world))
        mean = self._loss_sum / self._micro
        self._micro = 0
        return mean


def fit(model, train_loader, val_loader=None, max_epochs: int = 1, max_steps: int = -1, log_every: int = 50,
        val_check_interval: float = 0.5, ckpt_dir: str | None = None, world: int = 1, rank: int = 0, log=print,
        callbacks=(), accumulate_grad_batches: int = 1, optimizer=None, start_epoch: int = 0, start_step: int = 0):
    """Minimal Trainer.fit: epochs over the loader, validation every ``val_check_interval`` of an epoch
    (scripts/train_trocr.py:174), rank-0 checkpoints named like the reference (:138).
    ``accumulate_grad_batches`` (Lightning's): one optimizer step per that many batches (``Stepper``); the global step, ``max_steps``
    and ``log_every`` count optimizer steps, validation intervals count batches.  ``optimizer``: the model's optimizer when the caller
    has already configured it (parameter groups, a resumed state); ``start_epoch`` / ``start_step``: where a resumed run continues."""
    import torch
    opt = optimizer if optimizer is not None else model.configure_optimizers()
    stepper = Stepper(model, opt, world=world, accumulate_grad_batches=accumulate_grad_batches)
    model.hparams.accumulate_grad_batches = stepper.accumulate_grad_batches
    for cb in callbacks:          # e.g. kzv.ema.EMACallback (scripts/train_trocr.py:154,182)
        cb.on_fit_start(model)
    gstep = int(start_step)
    history = []
    best, save_top_k = [], 3          # (val_loss, path) of the kept checkpoints
    fit.best_model_path = None
    n_batches = len(train_loader)
    val_every = max(1, int(n_batches * val_check_interval)) if val_loader is not None else 0
    for epoch in range(int(start_epoch), max_epochs):
        if hasattr(train_loader, "set_epoch"):
            train_loader.set_epoch(epoch)          # DataLoader(shuffle=True) / DistributedSampler.set_epoch: a new order per epoch
        model.train()
        model.on_train_epoch_start()
        t0 = time.time()
        for i, batch in enumerate(train_loader):
            loss = stepper.step(batch, i, last_batch=i == n_batches - 1)
            if stepper.stepped:
                gstep += 1
                for cb in callbacks:
                    cb.on_train_batch_end(model)
            if stepper.stepped and (gstep % log_every == 0 or gstep == 1):
                lv = float(loss.item())
                history.append((gstep, lv))
                if rank == 0:
                    log(f"epoch {epoch} step {gstep} train_loss {lv:.4f} lr {opt.scheduled_lr:.3g}")
            if val_every and (i + 1) % val_every == 0:
                model.on_validation_epoch_start()
                for cb in callbacks:
                    cb.on_validation_start(model)
                vals = [model.validation_step(vb, j) for j, vb in enumerate(val_loader)]
                for cb in callbacks:
                    cb.on_validation_end(model)
                model.on_validation_epoch_end()
                model.train()
                vl = sum(vals) / max(1, len(vals))
                if rank == 0:
                    log(f"epoch {epoch} step {gstep} val_loss {vl:.4f}")
                    if ckpt_dir:
                        # ModelCheckpoint(monitor="val_loss", save_top_k=3) of scripts/train_trocr.py:136-143: keep the three
                        # best, write only when the new one ranks among them
                        if len(best) < save_top_k or vl < best[-1][0]:
                            os.makedirs(ckpt_dir, exist_ok=True)
                            path = os.path.join(ckpt_dir, f"trocr-epoch={epoch:02d}-val_loss={vl:.2f}.ckpt")
                            k = 1
                            while os.path.exists(path):        # Lightning's -v1, -v2 suffixes for equal names
                                path = os.path.join(ckpt_dir, f"trocr-epoch={epoch:02d}-val_loss={vl:.2f}-v{k}.ckpt"); k += 1
                            save_checkpoint(model, opt, path, epoch, gstep, callbacks)
                            best.append((vl, path)); best.sort(key=lambda e: e[0])
                            for _, stale in best[save_top_k:]:
                                if os.path.exists(stale):
                                    os.remove(stale)
                            del best[save_top_k:]
                            fit.best_model_path = best[0][1]
            if 0 < max_steps <= gstep:
                break
        torch.cuda.synchronize()
        if rank == 0:
            log(f"epoch {epoch} done in {time.time() - t0:.1f}s")
        if 0 < max_steps <= gstep:
            break
    if ckpt_dir and rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
        save_checkpoint(model, opt, os.path.join(ckpt_dir, "last.ckpt"), max_epochs - 1, gstep, callbacks)
        if fit.best_model_path is None:            # no validation ran: "best" falls back to the last weights, like Lightning
            fit.best_model_path = os.path.join(ckpt_dir, "last.ckpt")
    return history


def save_checkpoint(model, opt, path: str, epoch: int, global_step: int, callbacks=(), spelling: str = "hf4") -> None:
    """What Lightning's ModelCheckpoint writes for the reference (scripts/train_trocr.py:136-143): state_dict under HF
    names in the reference's order, schedulefree's per-parameter optimizer state, hyper_parameters -- kzv/checkpoint.py."""
    import torch
    from .checkpoint import build_checkpoint
    ck = build_checkpoint(model.cfg, model.flat_params.detach().cpu(), vars(model.hparams), epoch, global_step,
                          optimizer=opt.state_dict() if opt is not None else None, spelling=spelling)
    for cb in callbacks:
        ck = cb.on_save_checkpoint(model, ck)
    torch.save(ck, path)


def load_checkpoint(model, opt, path: str, callbacks=()):
    """Load a checkpoint written by this engine OR by the reference under Lightning (either ViT key spelling; optimizer
    state mapped through the checkpoint's own parameter order)."""
    import torch
    from .checkpoint import read_checkpoint
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd, osd = read_checkpoint(ck, model.cfg)
    model.load_state_dict(sd, strict=True)
    # the training criterion travels with the weights; a checkpoint without the key (every reference checkpoint) means the plain loss
    hp = ck.get("hyper_parameters") or {}
    def hparam(name, default):
        return hp.get(name, default) if isinstance(hp, dict) else getattr(hp, name, default)
    model.focal_gamma = 0.0                     # (first: the two setters refuse a gamma > 0 beside an eps > 0, in either order)
    model.label_smoothing = float(hparam("label_smoothing", 0.0))
    model.focal_gamma = float(hparam("focal_gamma", 0.0))
    model.class_weights = hparam("class_weights", None)
    # so do the fine-tuning settings (kzv/finetune.py): frozen layers on the model, the group table on the optimizer; no keys = off
    from . import finetune
    ft = finetune.settings_from_hparams(hp)
    model.hparams.accumulate_grad_batches = ft.pop("accumulate_grad_batches")
    finetune.apply(model, opt, **ft)
    if opt is not None and osd is not None:
        opt.load_state_dict(osd)
    for cb in callbacks:
        cb.on_load_checkpoint(model, ck)
    return ck


def test(model, test_loader, ckpt_path: str | None = None, log=print, rank: int = 0, stream_decode: bool | str = False, n_best: int = 0):
    """``trainer.test(model, test_loader, ckpt_path="best")`` (scripts/train_trocr.py:193-195): load the best checkpoint,
    switch the optimizer to its eval parameters (on_test_epoch_start, trocr_model.py:441-445), run test_step over the
    loader, report the epoch means of test_loss / test_cer.  ``stream_decode`` (an extension): True also reports ``test_cer_greedy``,
    the mean CER of ONE slot-refill greedy decode over the whole loader (``generate_stream``); "stream-beam" instead reports
    ``test_cer_stream_beam`` from ONE ``generate_stream(num_beams=4)`` over it, test_step's own decode on refilled slots; test_step
    itself is untouched.  In the stream modes, where the tokenizer is one character per token (``model.one_char_tokenizer``), the
    per-line values are computed from the ids on the device (kzv.metrics.edit_stats: the same values, ==) and rank 0 logs one more
    line: substitutions / deletions / insertions, corpus CER and the ten characters with the most errors; other tokenizers keep
    batch_decode + calculate_cer.  ``n_best`` n in 1..4 (with "stream-beam"; an extension): that decode returns the n best readings of every
    line (``generate_stream(num_return_sequences=n)``), ``test_cer_stream_beam`` stays the winners', and the call also reports
    ``test_cer_oracle`` -- the mean CER of each line's best reading, what a rescoring of the candidates could reach at most -- and rank 0
    logs how often each rank held it (kzv.nbest.oracle_stats)."""
    if n_best and stream_decode != "stream-beam":
        raise ValueError("trainer.test: n_best needs stream_decode=\"stream-beam\" (an n-best list comes from the beam search on refilled slots)")
    if ckpt_path:
        load_checkpoint(model, model.optimizers(), ckpt_path)
    model.eval()
    model.on_test_epoch_start()
    model.logged.pop("test_loss", None); model.logged.pop("test_cer", None)
    for j, b in enumerate(test_loader):
        model.test_step(b, j)
    keys = ("test_loss", "test_cer")
    detail = None
    if stream_decode and model.tokenizer is not None:
        import torch
        key, kw = ("test_cer_stream_beam", {"num_beams": 4, "early_stopping": True}) if stream_decode == "stream-beam" else ("test_cer_greedy", {})
        model.logged.pop(key, None)
        gen_all = None
        if n_best:
            model.logged.pop("test_cer_oracle", None)
            gen_all = model.generate_stream((b["pixel_values"] for b in test_loader), **kw, num_return_sequences=int(n_best), **getattr(model, "decode_controls", {}))
            gen = gen_all[0::int(n_best)]
        else:
            gen = model.generate_stream((b["pixel_values"] for b in test_loader), **kw, **getattr(model, "decode_controls", {}))
        labels = torch.cat([b["labels"] for b in test_loader])
        from . import metrics as M
        if model.one_char_tokenizer and gen.shape[1] <= M.MAX_WIDTH and labels.shape[1] <= M.MAX_WIDTH:
            # one character per token: the same per-line values from the ids, on the device (include/kzv.h: kzv_edit_distance)
            st = M.edit_stats(gen, labels.to(gen.device), model.tokenizer.all_special_ids, model.cfg.vocab, char_stats=True)
            for v in M.cer_values(st["dist"], st["ref_len"], st["pred_len"]):
                model.log(key, v)
            detail = _edit_detail(M, st, model.tokenizer)
        else:
            preds = model.tokenizer.batch_decode(gen, skip_special_tokens=True)
            tgts = model.tokenizer.batch_decode(labels, skip_special_tokens=True)
            for p, t in zip(preds, tgts):
                model.log(key, model.calculate_cer(p, t))
        keys += (key,)
        if gen_all is not None:
            import numpy as np
            from . import nbest as NB
            n = int(n_best)
            if model.one_char_tokenizer and gen_all.shape[1] <= M.MAX_WIDTH and labels.shape[1] <= M.MAX_WIDTH:
                st2 = M.edit_stats(gen_all, labels.to(gen_all.device).repeat_interleave(n, dim=0), model.tokenizer.all_special_ids, model.cfg.vocab, ops=False)
                d, r, q = (st2[k].view(-1, n).cpu().numpy() for k in ("dist", "ref_len", "pred_len"))
            else:
                hyps = model.tokenizer.batch_decode(gen_all, skip_special_tokens=True)
                tgts = [t for t in model.tokenizer.batch_decode(labels, skip_special_tokens=True) for _ in range(n)]
                from .model import _levenshtein
                d = np.asarray([_levenshtein(h, t) for h, t in zip(hyps, tgts)]).reshape(-1, n)
                r = np.asarray([len(t) for t in tgts]).reshape(-1, n)
                q = np.asarray([len(h) for h in hyps]).reshape(-1, n)
            oracle = NB.oracle_stats(d, r[:, 0], q)
            for v in oracle["cer_oracle_lines"]:
                model.log("test_cer_oracle", v)
            keys += ("test_cer_oracle",)
            detail = (detail + "\n" if detail else "") + "best reading at rank (0 = the winner): " + " ".join(f"{k}:{c}" for k, c in enumerate(oracle["oracle_rank"]))
    if model.optimizers() is not None:
        model.optimizers().train()
    out = {k: (sum(model.logged[k]) / len(model.logged[k]) if model.logged.get(k) else float("nan")) for k in keys}
    if rank == 0:
        log(" ".join(f"{k} {out[k]:.4f}" for k in keys))
        if detail:
            log(detail)
    return out


def _edit_detail(M, st, tokenizer) -> str:
    """One line for the log: substitutions / deletions / insertions, corpus CER and the ten characters with the most errors."""
    ops = st["ops"].sum(dim=0).tolist()
    chars, dist = int(st["ref_len"].sum()), int(st["dist"].sum())
    worst = " ".join(f"{r['char']}:{r['substituted'] + r['deleted'] + r['inserted']}/{r['count']}"
                     for r in M.character_table(st["char_stats"], tokenizer, top=10) if r["substituted"] + r["deleted"] + r["inserted"])
    return (f"edits S {ops[1]} D {ops[2]} I {ops[3]} over {chars} label characters, corpus CER "
            f"{dist / chars if chars else 0.0:.4f}; most errors (errors/occurrences): {worst or '-'}")
