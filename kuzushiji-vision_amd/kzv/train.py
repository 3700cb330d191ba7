#!/usr/bin/env python3
"""CLI entrypoint of the MI355X engine: the flag surface of scripts/train_trocr.py:23-71 (TrOCR) plus the
ocr_lightning/train.py:161-189 spellings, wired to kzv.TrOCRModel + kzv.trainer.fit; `--model ocr` trains ocr_lightning/model.py's
ResNet34 / BiLSTM / CTC OCRModel (kzv.ocr_model) on ocr_lightning/train.py's folder datasets.

  python -m kzv.train --synthetic 64 --batch_size 32 --encoder_hidden_size 384 --encoder_num_layers 6 \
         --encoder_num_heads 6 --image_size 64 640 --max_epochs 1            # BASELINE.json configs[0] plumbing
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m kzv.train --gpus 8 ...
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Train TrOCR model (MI355X engine)")
    # data (scripts/train_trocr.py:27-36)
    p.add_argument("--csv_path", type=str, default="data/processed_v2/column_info.csv")
    p.add_argument("--image_root", type=str, default="data/processed_v2/column_images")
    p.add_argument("--decoder_path", type=str,
                   default="experiments/pretrain_language_model/roberta-small-japanese-aozora-char/20250530_034458/checkpoint-200000")
    p.add_argument("--synthetic", type=int, default=0, help="train on N synthetic line crops (no CSV / checkpoint needed)")
    p.add_argument("--train_data_dir", type=str, default=None, help="ocr_lightning/train.py spelling (unused by TrOCR)")
    p.add_argument("--val_data_dir", type=str, default=None, help="ocr_lightning/train.py spelling (unused by TrOCR)")
    # model (:39-44)
    p.add_argument("--image_size", type=int, nargs=2, default=[1024, 64])
    p.add_argument("--patch_size", type=int, nargs=2, default=[16, 16])
    p.add_argument("--encoder_hidden_size", type=int, default=768)
    p.add_argument("--encoder_num_layers", type=int, default=12)
    p.add_argument("--encoder_num_heads", type=int, default=8,
                   help="reference default 8 = head_dim 96 (scripts/train_trocr.py:43); head_dim 64 and 96 run on MFMA attention kernels "
                        "(whole-head up to 288 tokens, K/V-streaming up to 4,097 = 4,096 patches + CLS), other multiples of 8 up to 128 "
                        "on a plain fp32 kernel, several times slower and for at most 287 patches")
    p.add_argument("--max_length", type=int, default=128)
    # training (:47-54)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--learning_rate", type=float, default=1e-4)
    p.add_argument("--weight_decay", type=float, default=0)
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--epsilon", type=float, default=1e-8)
    p.add_argument("--max_epochs", type=int, default=50)
    p.add_argument("--max_steps", type=int, default=-1)
    p.add_argument("--num_workers", type=int, default=8)
    p.add_argument("--train_ratio", type=float, default=0.8)
    p.add_argument("--val_ratio", type=float, default=0.1)
    p.add_argument("--test_ratio", type=float, default=0.1)
    # output (:62-63)
    p.add_argument("--output_dir", type=str, default="experiments/trocr")
    p.add_argument("--experiment_name", type=str, default="trocr_vit_roberta")
    # hardware (:66-69 and ocr_lightning/train.py:182-186)
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--devices", type=str, default=None, help="ocr_lightning spelling of --gpus")
    p.add_argument("--accelerator", type=str, default="gpu")
    p.add_argument("--precision", type=str, default="bf16-mixed", choices=["16-mixed", "32", "bf16-mixed", "fp8-mixed"],
                   help="bf16-mixed = the reference's setting and this engine's arithmetic; fp8-mixed (an extension, BASELINE configs[4]) "
                        "additionally runs the encoder's QKV / fc1 / fc2 forward GEMMs on e4m3 operands (hidden and ffn sizes must be multiples of 256)")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--decode_weights", type=str, default="bf16", choices=["bf16", "e4m3"],
                   help="e4m3 (an extension): validation / test decodes read the decoder's streamed linears as e4m3 with a power-of-two "
                        "scale per output row where the one-launch generation step runs (kzv.quant states what that equals); training is untouched")
    p.add_argument("--test_decode", type=str, default="beam", choices=["beam", "stream", "stream-beam"],
                   help="stream (an extension): the test phase also logs test_cer_greedy from ONE slot-refill greedy decode over the whole test "
                        "loader (TrOCRModel.generate_stream); stream-beam (an extension): it also logs test_cer_stream_beam from ONE "
                        "generate_stream(num_beams=4) over it, the test step's own beam search on refilled slots; beam = the reference's test "
                        "phase alone")
    p.add_argument("--test_n_best", type=int, default=0,
                   help="with --test_decode stream-beam (an extension): that decode returns the N best readings of every line (1..4, "
                        "generate_stream(num_return_sequences=N)) and the test phase also logs test_cer_oracle, the mean CER of each line's "
                        "best reading -- what a language model or lexicon rescoring of the candidates could reach at most -- and how often "
                        "each rank held it; 0 = off")
    p.add_argument("--no_repeat_ngram_size", type=int, default=0,
                   help="generation control of the validation / test decodes (an extension; transformers.generate's name and rule): no "
                        "n-gram of this size occurs twice in a decoded line; 0 = off, the reference's behaviour")
    p.add_argument("--repetition_penalty", type=float, default=1.0,
                   help="generation control of the validation / test decodes: scores of tokens already emitted are divided by it (multiplied "
                        "where negative); 1.0 = off, the reference's behaviour")
    p.add_argument("--min_length", type=int, default=0,
                   help="generation control of the validation / test decodes: no EOS before a line holds this many tokens, BOS included; "
                        "0 = off, the reference's behaviour")
    p.add_argument("--lm_path", type=str, default=None,
                   help="character n-gram language model fused into the validation / test decodes (an extension; kzv.lm): an .npz written by "
                        "kzv.lm, or an ARPA file by its .arpa extension (KenLM / SRILM)")
    p.add_argument("--lm_order", type=int, default=0,
                   help="with N > 0 and no --lm_path: fit an order-N model (1..4) on the training split's label ids at start-up and save it as "
                        "lm.npz beside the checkpoints; 0 = off")
    p.add_argument("--lm_weight", type=float, default=0.0,
                   help="weight of the language model's log-probability in every decode step's scores (shallow fusion, after the generation "
                        "controls); 0.0 = off, the reference's behaviour")
    p.add_argument("--device_preprocess", action="store_true",
                   help="resize / pad / normalise the decoded crops on the GPU (kzv.preprocess; byte-exact with the PIL transform)")
    p.add_argument("--augment", type=str, default="off", choices=["off", "reference"],
                   help="training-time augmentation of the crops on the GPU (an extension; kzv.augment): reference = the reference workspace's "
                        "own numbers (RandomAffine 7 deg / 7 %% / 0.93-1.07 / shear 5, brightness-contrast, noise, blur, stroke thinning and "
                        "thickening); validation and test batches are never augmented; off = the crops as they lie on disk")
    p.add_argument("--augment_seed", type=int, default=None, help="seed of the augmentation draws (default: --seed)")
    p.add_argument("--label_smoothing", type=float, default=0.0,
                   help="label smoothing of the TrOCR training loss (an extension; nn.CrossEntropyLoss(label_smoothing=...), 0 <= value < 1; "
                        "the published TrOCR recipe uses 0.1): train_loss in the logs is then the SMOOTHED loss, while val_loss and the test "
                        "losses stay the plain cross-entropy, so checkpoints rank and runs compare as without it; the value is written into "
                        "the checkpoints' hyper_parameters; 0 = off, the reference's criterion")
    p.add_argument("--class_weights", type=str, default="none", metavar="{none,inv_sqrt,effective,PATH.npy}",
                   help="per-class weights of the TrOCR training loss (an extension; nn.CrossEntropyLoss(weight=...)) for the long tail of the "
                        "vocabulary, from how often each character is a target in the training split: inv_sqrt = count ** -0.5, effective = "
                        "(1 - beta) / (1 - beta ** count) (class-balanced loss), both clamped to --class_weight_cap and scaled so that an "
                        "average training token weighs 1; PATH.npy = float32 weights [vocab] of your own (kzv.classweights builds them); "
                        "train_loss in the logs is then the WEIGHTED loss, while val_loss and the test losses stay the plain "
                        "cross-entropy, so checkpoints rank and runs compare as without it; the weights are written into the checkpoints' "
                        "hyper_parameters; none = off, the reference's criterion")
    p.add_argument("--class_weight_beta", type=float, default=0.999, help="beta of --class_weights effective, in (0, 1)")
    p.add_argument("--class_weight_cap", type=float, default=10.0,
                   help="largest ratio between two weights of --class_weights inv_sqrt / effective (>= 1): rarer classes are clamped to it")
    p.add_argument("--focal_gamma", type=float, default=0.0,
                   help="focal modulation of the TrOCR training loss (an extension): every target's loss is scaled by (1 - p_target) ** gamma, "
                        "0 <= gamma <= 5, so characters the model already gets right count less; combines with --class_weights, not with "
                        "--label_smoothing; train_loss in the logs is then the FOCAL loss, while val_loss and the test losses stay the "
                        "plain cross-entropy; 0 = off, the reference's criterion")
    p.add_argument("--skip_test", action="store_true", help="do not run the reference's post-fit test phase (scripts/train_trocr.py:193-195)")
    p.add_argument("--ema_decay", type=float, default=0.0, help="> 0 attaches kzv.ema.EMACallback (reference: decay 0.9999)")
    # the ResNet34 / BiLSTM / CTC model of ocr_lightning/model.py behind ocr_lightning/train.py's own flags (:161-189)
    p.add_argument("--model", type=str, default="trocr", choices=["trocr", "ocr"],
                   help="trocr = scripts/train_trocr.py's model (the benchmark path); ocr = ocr_lightning/train.py's OCRModel "
                        "(--train_data_dir / --val_data_dir folder datasets, Adam, early stopping on val/total_loss)")
    p.add_argument("--checkpoint_dir", type=str, default="./ocr_checkpoints")
    p.add_argument("--log_dir", type=str, default="./ocr_logs")
    p.add_argument("--max_boxes", type=int, default=50)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--patience", type=int, default=3)
    p.add_argument("--resume", type=str, default=None,
                   help="continue from a checkpoint this CLI (or Lightning, for the reference) wrote (pl.Trainer.fit(ckpt_path=...)): "
                        "--model ocr: weights, Adam moments and step count, epoch; TrOCR: weights, optimizer state, epoch and global step, and "
                        "the checkpoint's fine-tuning settings where the flags below are left at their defaults")
    # fine-tuning (extensions; kzv/finetune.py), TrOCR only
    p.add_argument("--init_from", type=str, default=None,
                   help="start from the WEIGHTS of a checkpoint (strict: every key, no other); the optimizer starts fresh, epoch and step at 0")
    p.add_argument("--freeze_encoder_layers", type=int, default=0,
                   help="freeze the patch embedding, the CLS token, the position table and encoder layers 0 .. N-1 (0 <= N <= "
                        "--encoder_num_layers): no backward, no optimizer traffic, no all-reduce for them; 0 = off")
    p.add_argument("--layer_decay", type=float, default=1.0,
                   help="layer-wise learning-rate decay (BEiT's): a parameter of encoder layer i trains with lr * D ** (layers - i), the "
                        "embeddings with D ** (layers + 1), the decoder with lr; 0 < D <= 1, 1 = off")
    p.add_argument("--decay_exempt", type=str, default="none", choices=["none", "bias_norm"],
                   help="bias_norm: no weight decay on biases, LayerNorm gains and the encoder's CLS and position tables")
    p.add_argument("--accumulate_grad_batches", type=int, default=1,
                   help="one optimizer step per K batches (Lightning's): gradients add up over K forward + backward passes and are divided by "
                        "K; --max_steps counts optimizer steps; 1 = off")
    args = p.parse_args(argv)
    if not 0.0 < args.layer_decay <= 1.0:
        p.error(f"--layer_decay must be in (0, 1], not {args.layer_decay}")
    if not 0 <= args.freeze_encoder_layers <= args.encoder_num_layers:
        p.error(f"--freeze_encoder_layers must be in 0..{args.encoder_num_layers} (--encoder_num_layers), not {args.freeze_encoder_layers}")
    if args.accumulate_grad_batches < 1:
        p.error(f"--accumulate_grad_batches must be >= 1, not {args.accumulate_grad_batches}")
    if args.init_from and args.resume:
        p.error("--init_from and --resume do not combine: one starts the optimizer fresh, the other continues it")
    if args.model == "ocr":
        for flag, on, why in (("--init_from", args.init_from, "--model ocr loads weights together with its Adam state: use --resume"),
                              ("--freeze_encoder_layers", args.freeze_encoder_layers, "--model ocr has no ViT encoder layers to freeze"),
                              ("--layer_decay", args.layer_decay != 1.0, "--model ocr has no ViT encoder whose layers a decay could follow"),
                              ("--decay_exempt", args.decay_exempt != "none", "--model ocr trains with torch's Adam, which has no parameter-range table"),
                              ("--accumulate_grad_batches", args.accumulate_grad_batches != 1, "--model ocr's step has no accumulation window")):
            if on:
                p.error(f"{flag} applies to the TrOCR model only: {why}")
    if args.test_n_best:
        if args.model == "ocr":
            p.error("--test_n_best acts on the TrOCR beam search only: --model ocr decodes with CTC, which keeps no list of hypotheses")
        if args.test_decode != "stream-beam":
            p.error("--test_n_best needs --test_decode stream-beam: the n-best list comes from the beam search on refilled slots")
        if not 1 <= args.test_n_best <= 4:
            p.error(f"--test_n_best must be in 1..4 (the test decode runs 4 beams), not {args.test_n_best}")
    if not 0.0 <= args.label_smoothing < 1.0:
        p.error(f"--label_smoothing must be in [0, 1), not {args.label_smoothing}")
    if args.label_smoothing and args.model == "ocr":
        p.error("--label_smoothing applies to the TrOCR cross-entropy only: --model ocr trains with CTC and SmoothL1 losses, which have no "
                "softmax cross-entropy to smooth")
    if not 0.0 <= args.focal_gamma <= 5.0:
        p.error(f"--focal_gamma must be in [0, 5], not {args.focal_gamma}")
    if args.focal_gamma > 0 and args.label_smoothing > 0:
        p.error("--focal_gamma and --label_smoothing do not combine: nobody has stated that loss; set one of them to 0")
    if args.class_weights not in ("none", "inv_sqrt", "effective") and not args.class_weights.endswith(".npy"):
        p.error(f"--class_weights must be none, inv_sqrt, effective or a .npy file, not {args.class_weights}")
    if not 0.0 < args.class_weight_beta < 1.0:
        p.error(f"--class_weight_beta must be in (0, 1), not {args.class_weight_beta}")
    if not args.class_weight_cap >= 1.0:
        p.error(f"--class_weight_cap must be >= 1, not {args.class_weight_cap}")
    if args.model == "ocr" and (args.class_weights != "none" or args.focal_gamma > 0 or args.class_weight_beta != 0.999 or args.class_weight_cap != 10.0):
        p.error("--class_weights / --class_weight_beta / --class_weight_cap / --focal_gamma apply to the TrOCR cross-entropy only: "
                "--model ocr trains with CTC and SmoothL1 losses")
    if args.model == "ocr" and (args.lm_path or args.lm_order or args.lm_weight):
        p.error("--lm_path / --lm_order / --lm_weight act on the TrOCR decodes only: --model ocr decodes with CTC, which has no "
                "step-wise scores to fuse a language model into")
    if not 0 <= args.lm_order <= 4:
        p.error(f"--lm_order must be in 0..4, not {args.lm_order}")
    if args.lm_weight != args.lm_weight or args.lm_weight in (float("inf"), float("-inf")):
        p.error("--lm_weight must be finite")
    return args


def _decode_lm(args, model, train_ds, out_dir, rank, world=1):
    """The language model of the validation / test decodes from --lm_path / --lm_order, said once.  With --lm_order N > 0 and no
    --lm_path the model is fitted on the training split's label ids -- by rank 0, which saves it as lm.npz beside the checkpoints; the
    other ranks load that file -- whatever the weight.  Returns None where --lm_weight is 0 (off) or no model was asked for.
    The tokenizer adds no BOS / EOS on encode and a decode's history starts with BOS, so every label row is wrapped as BOS ... EOS."""
    from . import lm as LM
    c = model.cfg
    if not (args.lm_path or args.lm_order):
        return None
    if args.lm_path:
        lm = LM.load_any(args.lm_path, model.tokenizer, c.bos_id, c.eos_id, c.vocab)
    else:
        path = os.path.join(out_dir, "checkpoints", "lm.npz")
        if rank == 0:
            if hasattr(train_ds, "data") and getattr(train_ds, "tokenizer", None) is not None:      # the texts, no image is opened
                rows = [train_ds.tokenizer(t, max_length=train_ds.max_length, truncation=True)["input_ids"] for t in train_ds.data["text"]]
            else:
                rows = [train_ds[i]["labels"].numpy() for i in range(len(train_ds))]
            seqs = LM.sequences_from_labels(rows, c.pad_id, c.eos_id, bos_id=c.bos_id)
            lm = LM.NGramLM.fit(seqs, args.lm_order, c.vocab)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            lm.save(path)
        if world > 1:
            import torch
            torch.distributed.barrier()              # rank 0 has written the file the others load
        if rank != 0:
            lm = LM.NGramLM.load(path)
    if rank == 0:
        print(f"language model: order {lm.order}, contexts {lm.n_contexts()}, weight {args.lm_weight}" + ("" if args.lm_weight else " (off)"))
    return lm if args.lm_weight else None


def _label_rows(train_ds):
    """The training split's label ids, row by row, without opening an image where the dataset keeps its texts."""
    if hasattr(train_ds, "data") and getattr(train_ds, "tokenizer", None) is not None:
        return [train_ds.tokenizer(t, max_length=train_ds.max_length, truncation=True)["input_ids"] for t in train_ds.data["text"]]
    return [train_ds[i]["labels"].numpy() for i in range(len(train_ds))]


def _class_weights(args, model, train_ds, rank):
    """The weights --class_weights asks for (None: off), said once.  Every rank derives the same weights from the same split."""
    import numpy as np
    from . import classweights as CW
    if args.class_weights == "none":
        return None
    c = model.cfg
    if args.class_weights.endswith(".npy"):
        w = np.load(args.class_weights).astype(np.float32).reshape(-1)
        what, cap = args.class_weights, None
    else:
        counts = CW.count_targets(_label_rows(train_ds), c.vocab, c.pad_id)
        if args.class_weights == "inv_sqrt":
            w = CW.from_counts(counts, "inv_pow", power=0.5, cap=args.class_weight_cap)
        else:
            w = CW.from_counts(counts, "effective", beta=args.class_weight_beta, cap=args.class_weight_cap)
        what, cap = f"{args.class_weights} over {int(counts.sum())} targets, {int((counts > 0).sum())} of {c.vocab} classes seen", args.class_weight_cap
    if rank == 0:
        print(f"class weights: {what}: {CW.describe(w, cap)} (train_loss is the weighted loss; val_loss stays the plain cross-entropy)")
    return w


def main_ocr(args):
    """ocr_lightning/train.py:35-158: seed, folder datasets + pad-collate loaders, OCRModel, ModelCheckpoint(monitor val/total_loss,
    save_top_k=1, save_last) + EarlyStopping(patience) over `--epochs` epochs of Adam steps; per-epoch metrics as JSON lines in --log_dir
    (the reference writes TensorBoard events; there is no tensorboard in this image)."""
    import json
    import torch
    from .ocr_data import CHAR_TO_IDX, IDX_TO_CHAR, OcrDataset, OcrLoader
    from .ocr_model import OCRModel
    if not args.train_data_dir or not args.val_data_dir:
        raise SystemExit("--model ocr needs --train_data_dir and --val_data_dir (ocr_lightning/train.py:163-164)")
    if args.accelerator not in ("gpu", "auto"):
        raise SystemExit("this engine runs on MI355X GPUs only")
    from .trainer import init_distributed
    rank, world, local = init_distributed()              # one process per GPU (torch.distributed.run), as for the TrOCR path
    torch.cuda.set_device(local)
    torch.manual_seed(args.seed)
    os.makedirs(args.checkpoint_dir, exist_ok=True); os.makedirs(args.log_dir, exist_ok=True)
    train_ds = OcrDataset(args.train_data_dir, char_to_idx=CHAR_TO_IDX)
    val_ds = OcrDataset(args.val_data_dir, char_to_idx=CHAR_TO_IDX)
    if len(train_ds) == 0:
        print(f"Error: Training dataset at {args.train_data_dir} is empty. Please check the path and data structure.")
        return None
    train_loader = OcrLoader(train_ds, args.batch_size, shuffle=True, seed=args.seed, rank=rank, world=world)
    val_loader = OcrLoader(val_ds, args.batch_size) if len(val_ds) else None
    model = OCRModel(CHAR_TO_IDX, IDX_TO_CHAR, learning_rate=args.learning_rate, max_boxes=args.max_boxes, init_seed=args.seed, device=f"cuda:{local}")
    model.configure_optimizers()
    start_epoch = 0
    if getattr(args, "resume", None):                       # what pl.Trainer.fit(ckpt_path=...) restores: weights, Adam state, epoch
        ck = torch.load(args.resume, map_location="cpu", weights_only=False)
        model.load_state_dict(ck["state_dict"], strict=True)
        if ck.get("optimizer_states"):
            model.load_optimizer_state_dict(ck["optimizer_states"][0])
        start_epoch = int(ck.get("epoch", -1)) + 1
        if rank == 0:
            print(f"Resumed from {args.resume}: epoch {start_epoch}, optimizer step {model._optimizer.step_count}")
    state, hist = {"best": float("inf"), "best_path": None, "bad": 0}, []
    log = open(os.path.join(args.log_dir, "metrics.jsonl") if rank == 0 else os.devnull, "a", encoding="utf-8")
    for epoch in range(start_epoch, args.epochs):
        train_loader.set_epoch(epoch)
        model.logged.clear()
        for i, batch in enumerate(train_loader):
            model.fit_step(batch, i)
        rec = {"epoch": epoch, **{k: sum(v) / len(v) for k, v in model.logged.items() if k.startswith("train/")}}
        if val_loader is not None:
            model.eval(); model.logged.clear()
            for i, batch in enumerate(val_loader):
                model.validation_step(batch, i)
            rec.update({k: sum(v) / len(v) for k, v in model.logged.items() if k.startswith("val/")})
            model.train()
        hist.append(rec)
        stop = [False]
        if rank == 0:
            stop[0] = _ocr_epoch_end(args, model, rec, epoch, log, state)
        if world > 1:                                        # every rank leaves the loop together (rank 0 monitors val/total_loss)
            torch.distributed.broadcast_object_list(stop, src=0)
        if stop[0]:
            break
    log.close()
    best_path = state["best_path"]
    if rank == 0:
        print(f"Training finished.\nBest model checkpoint saved at: {best_path}" if best_path else "No best model checkpoint was saved.")
    main_ocr.best_model_path = best_path
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    return hist


def _ocr_epoch_end(args, model, rec, epoch, log, state):
    """rank 0: metrics line, last.ckpt, ModelCheckpoint(monitor val/total_loss, save_top_k=1), EarlyStopping(patience) -> stop?"""
    import json
    import torch
    best, best_path, bad = state["best"], state["best_path"], state["bad"]
    log.write(json.dumps(rec) + "\n"); log.flush()
    print(" ".join(f"{k}={v:.4f}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items()))
    def ckpt():      # Lightning's layout for the keys the reference's checkpoints carry (ModelCheckpoint(save_last=True), train.py:118-126)
        return {"state_dict": {k: v.cpu() for k, v in model.state_dict().items()}, "hyper_parameters": vars(model.hparams), "epoch": epoch,
                "global_step": model._optimizer.step_count if model._optimizer else 0, "optimizer_states": [model.optimizer_state_dict()], "lr_schedulers": []}
    torch.save(ckpt(), os.path.join(args.checkpoint_dir, "last.ckpt"))
    vl = rec.get("val/total_loss")
    if vl is not None:
        if vl < best:
            best, bad = vl, 0
            if best_path and os.path.exists(best_path):
                os.remove(best_path)
            best_path = os.path.join(args.checkpoint_dir, f"ocr-epoch={epoch:02d}-val_total_loss={vl:.2f}.ckpt")
            torch.save(ckpt(), best_path)
        else:
            bad += 1
            if bad >= args.patience:
                print(f"Early stopping: val/total_loss has not improved for {bad} epochs")
                state.update(best=best, best_path=best_path, bad=bad)
                return True
    state.update(best=best, best_path=best_path, bad=bad)
    return False


def main(argv=None):
    args = parse_args(argv)
    if args.model == "ocr":
        if args.augment != "off":
            raise SystemExit("--augment applies to the TrOCR line crops only: --model ocr trains on whole pages with box targets, which a "
                             "warp of the pixels alone would leave behind")
        return main_ocr(args)
    import torch
    from .config import ModelConfig
    from .data import LineCsvDataset, SyntheticLineDataset, build_decoder_dir, make_loader
    from .model import TrOCRModel
    from .trainer import fit, init_distributed, test as run_test

    if args.devices is not None:
        args.gpus = int(args.devices) if str(args.devices).isdigit() else len(str(args.devices).split(","))
    if args.accelerator != "gpu" or args.gpus < 1:
        raise SystemExit("this engine runs on MI355X GPUs only (the reference CPU Trainer branch is not provided)")
    if args.precision not in ("bf16-mixed", "fp8-mixed"):
        raise SystemExit("the engine implements bf16-mixed (scripts/train_trocr.py:68 default) and its fp8-mixed extension only")
    hd = args.encoder_hidden_size / max(1, args.encoder_num_heads)
    if hd != int(hd) or int(hd) % 8 or hd > 128:
        raise SystemExit(f"encoder head_dim {hd:g} is not supported: --encoder_hidden_size / --encoder_num_heads must be a multiple of 8 up to 128")
    if len(args.patch_size) == 2 and min(args.patch_size) > 0 and args.image_size[0] % args.patch_size[0] == 0 and args.image_size[1] % args.patch_size[1] == 0:
        tokens = (args.image_size[0] // args.patch_size[0]) * (args.image_size[1] // args.patch_size[1]) + 1
        if tokens > 288 and int(hd) not in (64, 96):
            raise SystemExit(f"--image_size {args.image_size[0]} {args.image_size[1]} with --patch_size {args.patch_size[0]} {args.patch_size[1]} "
                             f"gives {tokens} encoder tokens; beyond 288 the attention runs on streaming kernels for head_dim 64 and 96 only, "
                             f"and this encoder's is {int(hd)} (--encoder_hidden_size / --encoder_num_heads)")
        if tokens > 4097:
            raise SystemExit(f"--image_size {args.image_size[0]} {args.image_size[1]} with --patch_size {args.patch_size[0]} {args.patch_size[1]} "
                             f"gives {tokens} encoder tokens; the attention kernels take at most 4,097 (4,096 patches + CLS)")
    rank, world, local = init_distributed()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one process per GPU with torch.distributed.run")
    torch.manual_seed(args.seed)
    out_dir = os.path.join(args.output_dir, args.experiment_name)
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        print(f"Output directory: {out_dir}\nDecoder path: {args.decoder_path}")
    tmp = None
    decoder_path = args.decoder_path
    if args.synthetic and not os.path.exists(decoder_path):
        tmp = tempfile.TemporaryDirectory()
        decoder_path = build_decoder_dir(os.path.join(tmp.name, "decoder"), ModelConfig(max_pos=max(128, args.max_length)))
    if not os.path.exists(decoder_path):
        raise FileNotFoundError(f"Decoder path not found: {decoder_path}")      # scripts/train_trocr.py:88-89
    encoder_config = {"image_size": tuple(args.image_size), "patch_size": tuple(args.patch_size), "num_channels": 3,
                      "hidden_size": args.encoder_hidden_size, "num_hidden_layers": args.encoder_num_layers,
                      "num_attention_heads": args.encoder_num_heads, "intermediate_size": args.encoder_hidden_size * 4,
                      "hidden_dropout_prob": 0.1, "attention_probs_dropout_prob": 0.1}   # :111-121
    model = TrOCRModel(encoder_config, decoder_path, learning_rate=args.learning_rate, beta1=args.beta1, beta2=args.beta2,
                       epsilon=args.epsilon, weight_decay=args.weight_decay, device=f"cuda:{local}", init_seed=args.seed,
                       fp8=args.precision == "fp8-mixed", long_sequences=True, decode_weights=args.decode_weights,
                       label_smoothing=args.label_smoothing, focal_gamma=args.focal_gamma)
    model._step_seed = 1_000_003 * rank
    model.decode_controls = {k: v for k, v, off in (("no_repeat_ngram_size", args.no_repeat_ngram_size, 0),
                                                    ("repetition_penalty", args.repetition_penalty, 1.0),
                                                    ("min_length", args.min_length, 0)) if v != off}
    if rank == 0:
        c = model.cfg
        print(f"encoder attention: {model.encoder_attention_impl} (head_dim {c.enc_hidden // c.enc_heads}, {c.enc_seq} tokens)")
        generate = model.generate

        def generate_and_report(*a, **kw):      # the first validation decode binds the model: say once which step it took
            out = generate(*a, **kw)
            print(f"decode step: {model.decode_step_impl}, decoder weights: {model.decode_weights_impl}")
            del model.generate
            return out
        model.generate = generate_and_report
    if args.synthetic:
        n_val = max(args.batch_size, args.synthetic // 10)
        train_ds = SyntheticLineDataset(model.cfg, args.synthetic, args.max_length, seed=args.seed)
        val_ds = SyntheticLineDataset(model.cfg, n_val, args.max_length, seed=args.seed + 1)
        test_ds = SyntheticLineDataset(model.cfg, n_val, args.max_length, seed=args.seed + 2)
    else:
        kw = dict(csv_path=args.csv_path, image_root=args.image_root, tokenizer=model.tokenizer, image_size=tuple(args.image_size),
                  max_length=args.max_length, train_ratio=args.train_ratio, val_ratio=args.val_ratio, test_ratio=args.test_ratio)
        kw["device_preprocess"] = args.device_preprocess
        train_ds, val_ds, test_ds = LineCsvDataset(split="train", **kw), LineCsvDataset(split="val", **kw), LineCsvDataset(split="test", **kw)
    model.class_weights = _class_weights(args, model, train_ds, rank)
    decode_lm = _decode_lm(args, model, train_ds, out_dir, rank, world)
    if decode_lm is not None:
        model.decode_controls.update(lm=decode_lm, lm_weight=args.lm_weight)
    pre = None
    if args.device_preprocess and not args.synthetic:
        from .preprocess import DevicePreprocessor
        pre = DevicePreprocessor(tuple(args.image_size), device=f"cuda:{local}")
    nw = 0 if args.synthetic else max(0, args.num_workers)      # decode (and, without --device_preprocess, resize) in worker processes
    aug = None
    if args.augment != "off":
        from .augment import DeviceAugment, preset
        aug = (DeviceAugment(f"cuda:{local}"), preset(args.augment), args.seed if args.augment_seed is None else args.augment_seed)
    if rank == 0:
        print(f"augmentation: {args.augment}" + (f" (seed {aug[2]}, training batches only)" if aug else ""))
        if args.label_smoothing:
            print(f"label smoothing: {args.label_smoothing} (train_loss is the smoothed loss; val_loss stays the plain cross-entropy)")
        if args.focal_gamma:
            print(f"focal loss: gamma {args.focal_gamma} (train_loss is the focal loss; val_loss stays the plain cross-entropy)")
    train_loader = make_loader(train_ds, args.batch_size, True, args.seed, rank, world, num_workers=nw, preprocessor=pre, augment=aug)
    val_loader = make_loader(val_ds, args.batch_size, False, args.seed, rank, world, num_workers=nw, preprocessor=pre)
    test_loader = make_loader(test_ds, args.batch_size, False, args.seed, rank, world, num_workers=nw, preprocessor=pre)   # scripts/train_trocr.py:93
    if rank == 0:
        print(f"Train samples: {len(train_ds)}\nVal samples: {len(val_ds)}\nTest samples: {len(test_ds)}\nParameters: {model.num_parameters():,}")
    cbs = []
    if args.ema_decay > 0:
        from .ema import EMACallback
        cbs.append(EMACallback(args.ema_decay))
    # fine-tuning: where the run starts (--init_from: weights; --resume: weights, optimizer state, epoch, step and the checkpoint's
    # fine-tuning settings) and what trains how (frozen layers on the model, the range table on the optimizer)
    from . import finetune
    from .trainer import load_checkpoint
    opt = model.configure_optimizers()
    start_epoch = start_step = 0
    ft = dict(layer_decay=args.layer_decay, freeze_encoder_layers=args.freeze_encoder_layers, decay_exempt=args.decay_exempt)
    accumulate = args.accumulate_grad_batches
    if args.init_from:
        from .checkpoint import read_checkpoint
        sd, _ = read_checkpoint(torch.load(args.init_from, map_location="cpu", weights_only=False), model.cfg)
        model.load_state_dict(sd, strict=True)
        opt.z.copy_(model.flat_params)              # a fresh optimizer: its z iterate starts at the loaded weights
        if rank == 0:
            print(f"Initialised the weights from {args.init_from}; the optimizer starts fresh")
    if args.resume:
        ck = load_checkpoint(model, opt, args.resume)
        start_epoch, start_step = int(ck.get("epoch", 0)), int(ck.get("global_step", 0))
        if finetune.is_default(**ft):               # flags left alone: the checkpoint's settings (load_checkpoint has applied them)
            ft = dict(layer_decay=model.hparams.layer_decay, freeze_encoder_layers=model.hparams.frozen_encoder_layers,
                      decay_exempt=model.hparams.decay_exempt)
        if accumulate == 1:
            accumulate = int(model.hparams.accumulate_grad_batches)
        if rank == 0:
            print(f"Resumed from {args.resume}: epoch {start_epoch}, global step {start_step}")
    groups = finetune.apply(model, opt, **ft)
    if rank == 0 and (groups is not None or accumulate != 1):
        print(finetune.summary(groups if groups is not None else [(0, model.flat_params.numel(), 1.0, 1.0)])
              + f"; accumulate_grad_batches {accumulate}")
    main.start = (start_epoch, start_step)
    hist = fit(model, train_loader, val_loader, max_epochs=args.max_epochs, max_steps=args.max_steps, log_every=50,
               val_check_interval=0.5, ckpt_dir=os.path.join(out_dir, "checkpoints"), world=world, rank=rank,
               callbacks=cbs, accumulate_grad_batches=accumulate, optimizer=opt, start_epoch=start_epoch, start_step=start_step)
    if rank == 0:
        print(f"Training completed! Checkpoints saved to: {os.path.join(out_dir, 'checkpoints')}")
    # scripts/train_trocr.py:193-195: if test_loader is not None: trainer.test(model, test_loader, ckpt_path="best")
    main.test_metrics = None
    if not args.skip_test and len(test_ds) > 0:
        if world > 1:
            torch.distributed.barrier()            # rank 0 has written the checkpoint the others load
        path = fit.best_model_path if rank == 0 else None
        if world > 1:
            box = [path]
            torch.distributed.broadcast_object_list(box, src=0)
            path = box[0]
        main.test_metrics = run_test(model, test_loader, ckpt_path=path, rank=rank, stream_decode={"stream": True, "stream-beam": "stream-beam"}.get(args.test_decode, False),
                                     **({"n_best": args.test_n_best} if args.test_n_best else {}))
    if world > 1:
        torch.distributed.destroy_process_group()
    if tmp is not None:
        tmp.cleanup()
    return hist


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
