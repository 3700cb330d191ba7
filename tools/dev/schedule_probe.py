"""dev: fixed small scenarios through every host schedule of csrc/model*.cpp, for comparing two builds of libkzv.so.

    python tools/dev/schedule_probe.py list
    [KZV_LIB=other/libkzv.so] python tools/dev/schedule_probe.py <scenario> [--out DIR]
    python tools/dev/schedule_probe.py compare DIR_A DIR_B [DIR_A2]      # outputs; DIR_A2: a second run of build A (its own spread)
    python tools/dev/schedule_probe.py traces DIR_A DIR_B                # <scenario>/..._kernel_trace.csv of rocprofv3 --kernel-trace

One scenario = one process (the library reads its KZV_* switches once).  Under the profiler:
    rocprofv3 --kernel-trace --output-format csv -d DIR/<scenario> -- python tools/dev/schedule_probe.py <scenario> --out DIR

Model: 2 encoder layers of 128 / 2 heads on a 64 x 64 image (16 patches), the reference decoder geometry 256 / 4 / 768 with 2 layers,
B = 4, L = 9, dropout on, fixed seeds.  The fp8 scenarios widen the encoder to 256 / 4 heads / FFN 512 (kzv_set_fp8 takes multiples of
256 only); "dec64" swaps in a 64 / 1 / 128 decoder (no fragment packs).  Training scenarios run forward + backward twice with the same
seed and keep both gradient sets; generation scenarios decode 4 tokens greedily with one kzv_decode_reorder, once with a vocabulary
that is a multiple of 4 (logits straight into the caller's buffer) and once with one that is not (padded scratch + copy).
"""
import csv
import glob
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "kuzushiji-vision_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# scenario -> (kind, environment, model options)
SCENARIOS = {
    "default": ("train", {}, {}),
    "dec_chain0": ("train", {"KZV_DEC_CHAIN": "0"}, {}),
    "dec_chain1": ("train", {"KZV_DEC_CHAIN": "1"}, {}),
    "head_ce0": ("train", {"KZV_HEAD_CE": "0"}, {}),
    "head_dgrad0": ("train", {"KZV_HEAD_DGRAD": "0"}, {}),
    "dec_dgrad0": ("train", {"KZV_DEC_DGRAD": "0"}, {}),
    "dec_dgrad_wide": ("train", {"KZV_DEC_DGRAD_WIDE": "1"}, {}),
    "dec_dgrad_wide_chain1": ("train", {"KZV_DEC_DGRAD_WIDE": "1", "KZV_DEC_CHAIN": "1"}, {}),     # the switch acts where the segments are off
    "pair1": ("train", {"KZV_PAIR": "1"}, {}),
    "side1": ("train", {"KZV_SIDE_STREAM": "1"}, {}),
    "side2": ("train", {"KZV_SIDE_STREAM": "2"}, {}),
    "fp8_1": ("train", {}, {"fp8": 1}),
    "fp8_2": ("train", {}, {"fp8": 2}),
    "dec64": ("train", {}, {"dec64": True}),
    "gen_one_launch": ("gen", {}, {}),
    "gen_fused_ln": ("gen", {"KZV_DECODE_ONE_LAUNCH": "0"}, {}),
    "gen_per_op": ("gen", {"KZV_DECODE_ONE_LAUNCH": "0", "KZV_DECODE_FUSE_LN": "0"}, {}),
    "gen_graph": ("gen", {}, {"graph": True}),
}
B, LBL = 4, 9


def _config(opts, vocab=300):
    from kzv.config import ModelConfig
    enc = dict(enc_hidden=256, enc_heads=4, enc_ffn=512) if opts.get("fp8") else dict(enc_hidden=128, enc_heads=2, enc_ffn=256)
    dec = dict(dec_hidden=64, dec_heads=1, dec_ffn=128) if opts.get("dec64") else dict(dec_hidden=256, dec_heads=4, dec_ffn=768)
    return ModelConfig(image_h=64, image_w=64, enc_layers=2, dec_layers=2, vocab=vocab, max_pos=40, **enc, **dec)


def _model(cfg, tmp, opts):
    from kzv.data import build_decoder_dir
    from kzv.model import TrOCRModel
    d = build_decoder_dir(os.path.join(tmp, f"dec{cfg.vocab}"), cfg)
    return TrOCRModel(cfg.encoder_config_dict(), d, init_seed=7, load_tokenizer=False, fp8=opts.get("fp8", 0))


def _sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_train(opts, out_dir, name):
    import numpy as np
    import torch
    from kzv.data import synthetic_batch
    cfg = _config(opts)
    res = {"logits": [], "loss": []}
    with tempfile.TemporaryDirectory() as tmp:
        m = _model(cfg, tmp, opts)
        px, lab = synthetic_batch(cfg, B, LBL, seed=3, min_chars=2, max_chars=LBL - 2)
        pxt, labt = torch.from_numpy(px).cuda(), torch.from_numpy(lab).cuda()
        m.train()
        grads = {}
        for run in (0, 1):
            # the logits of a full-length forward (the GEMM + cross-entropy head), then the training step proper (no logits: the one-launch
            # head where it is on) and its backward, all with one seed
            _, logits = m.forward_loss(pxt, labt, want_logits=True, seed=11)
            torch.cuda.synchronize()
            res["logits"].append(_sha(logits))
            loss, _ = m.forward_loss(pxt, labt, want_logits=False, seed=11)
            m.backward()
            torch.cuda.synchronize()
            res["loss"].append(float(loss.item()).hex())
            for k, v in m.grad_dict().items():
                grads[f"{run}:{k}"] = v.detach().cpu().numpy().copy()
        np.savez(os.path.join(out_dir, name + ".grads.npz"), **grads)
    return res


def run_gen(opts, out_dir, name):
    import torch
    from kzv import _lib as L
    from kzv.data import synthetic_batch
    lib = L.load()
    res = {"tokens": [], "logits": []}
    steps, Lh = 4, 5                        # T = 4 cache positions: steps 0..3
    for vocab in (300, 301):
        cfg = _config(opts, vocab)
        with tempfile.TemporaryDirectory() as tmp:
            m = _model(cfg, tmp, opts)
            px, _ = synthetic_batch(cfg, B, LBL, seed=3, min_chars=2, max_chars=LBL - 2)
            m.eval()
            pxt = m._check_inputs(torch.from_numpy(px))
            stream = torch.cuda.Stream() if opts.get("graph") else torch.cuda.current_stream()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                ids = torch.full((B, Lh), cfg.pad_id, dtype=torch.int64, device="cuda")
                ids[:, 0] = cfg.bos_id
                logits = torch.empty(B, cfg.vocab, dtype=torch.float32, device="cuda")
                valid = torch.zeros(B, Lh, dtype=torch.uint8, device="cuda")
                posids = torch.empty(B, dtype=torch.int32, device="cuda")
                tok = torch.empty(B, dtype=torch.int64, device="cuda")
                rows = torch.tensor([1, 0, 3, 2], dtype=torch.int64, device="cuda")
                m._bind(B, Lh)
                st = L.stream_handle()
                L.check(lib.kzv_encode_images(m._h, pxt.data_ptr(), B, st), "encode_images")
                L.check(lib.kzv_set_active_length(m._h, 1), "set_active_length")
                L.check(lib.kzv_decode_begin(m._h, st), "decode_begin")
                digest = hashlib.sha256()
                for t in range(steps):
                    L.check(lib.kzv_decode_prep(ids.data_ptr(), ids.stride(0), t, cfg.pad_id, B, tok.data_ptr(), valid.data_ptr(), Lh, posids.data_ptr(), st), "decode_prep")
                    if opts.get("graph"):
                        L.check(lib.kzv_decode_step_graph(m._h, tok.data_ptr(), posids.data_ptr(), valid.data_ptr(), Lh, logits.data_ptr(), st), "decode_step_graph")
                    else:
                        L.check(lib.kzv_decode_step(m._h, tok.data_ptr(), posids.data_ptr(), t, valid.data_ptr(), Lh, logits.data_ptr(), st), "decode_step")
                    stream.synchronize()
                    digest.update(logits.cpu().numpy().tobytes())
                    ids[:, t + 1] = logits.argmax(dim=-1)
                    if t == 1:              # every sequence continues from its neighbour's cache rows (what a beam step does)
                        ids = ids[rows].contiguous()
                        valid.copy_(valid[rows])
                        L.check(lib.kzv_decode_reorder(m._h, rows.data_ptr(), t + 1, st), "decode_reorder")
                stream.synchronize()
            res["impl"] = m.decode_step_impl
            res["tokens"].append(ids.cpu().tolist())
            res["logits"].append(digest.hexdigest())
    return res


def _rel(a, b):
    import numpy as np
    return float(np.abs(a - b).max() / (np.abs(a).max() + 1e-30))


def compare(dir_a, dir_b, dir_a2=None):
    """Logits / loss / tokens bit for bit; per parameter, B's gradients against A's within twice A's own spread: the larger of the
    difference between A's two in-process runs and (with DIR_A2) the difference between A's two processes."""
    import numpy as np
    bad = 0
    for name in SCENARIOS:
        fa, fb = (os.path.join(d, name + ".json") for d in (dir_a, dir_b))
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print(f"{name}: missing"); bad += 1
            continue
        ja, jb = json.load(open(fa)), json.load(open(fb))
        line = {k: ja[k] == jb[k] for k in ja if k != "scenario"}
        self_same = all(len(set(map(str, v))) == 1 for k, v in ja.items() if k in ("logits", "loss")) if "loss" in ja else None
        msg = f"{name}: " + " ".join(f"{k} {'same' if v else 'DIFFERENT'}" for k, v in line.items())
        bad += sum(not v for v in line.values())
        ga = os.path.join(dir_a, name + ".grads.npz")
        if os.path.exists(ga):
            A, Bn = np.load(ga), np.load(os.path.join(dir_b, name + ".grads.npz"))
            A2 = np.load(os.path.join(dir_a2, name + ".grads.npz")) if dir_a2 and os.path.exists(os.path.join(dir_a2, name + ".grads.npz")) else None
            worst_own = worst_b = 0.0
            over = []
            for k in A.files:
                if not k.startswith("0:"):
                    continue
                own = _rel(A[k], A["1:" + k[2:]])
                if A2 is not None:
                    own = max(own, _rel(A[k], A2[k]))
                db = max(_rel(A[k], Bn[k]), _rel(A["1:" + k[2:]], Bn["1:" + k[2:]]))
                worst_own, worst_b = max(worst_own, own), max(worst_b, db)
                if db > 2 * own:
                    over.append((k[2:], own, db))
            msg += f" | grads: A's own spread {worst_own:.3g}, B against A {worst_b:.3g}, parameters beyond 2x their own spread: {len(over)}"
            for k, own, db in over[:6]:
                msg += f"\n      {k}: own {own:.3g} B {db:.3g}"
            bad += len(over)
            msg += f" | A reproduces its logits and loss in-process: {self_same}"
        print(msg)
    print("PROBE_COMPARE", "OK" if not bad else f"{bad} differences")
    return 1 if bad else 0


def _trace(d, name):
    files = glob.glob(os.path.join(d, name, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    for f in files:
        rows += list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    cols = ("Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size", "Queue_Id")
    return [tuple(r.get(c, "") for c in cols) for r in rows]


def traces(dir_a, dir_b):
    """The ordered (kernel, grid, workgroup, LDS) list per scenario, in dispatch order; where two streams are in use also per queue."""
    bad = 0
    for name in SCENARIOS:
        ta, tb = _trace(dir_a, name), _trace(dir_b, name)
        if ta is None or tb is None:
            print(f"{name}: missing trace"); bad += 1
            continue
        la, lb = [r[:-1] for r in ta], [r[:-1] for r in tb]
        if la == lb:
            print(f"{name}: {len(la)} launches, identical in order")
            continue
        # two streams: the dispatch ids of the two queues interleave as the runtime pleases; each stream's own order is what the host issued
        qa, qb = {}, {}
        for t, q in ((ta, qa), (tb, qb)):
            for r in t:
                q.setdefault(r[-1], []).append(r[:-1])
        per_queue = sorted(map(tuple, qa.values())) == sorted(map(tuple, qb.values()))
        first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
        print(f"{name}: {len(la)} vs {len(lb)} launches, DIFFERENT from launch {first}; per queue identical: {per_queue}; same multiset: {sorted(la) == sorted(lb)}")
        if first < min(len(la), len(lb)):
            print("     A:", la[first], "\n     B:", lb[first])
        bad += 0 if per_queue and len(qa) > 1 else 1
    print("PROBE_TRACES", "OK" if not bad else f"{bad} scenarios differ")
    return 1 if bad else 0


def main(argv):
    if not argv or argv[0] == "list":
        print(" ".join(SCENARIOS))
        return 0
    if argv[0] == "compare":
        return compare(*argv[1:4])
    if argv[0] == "traces":
        return traces(argv[1], argv[2])
    name = argv[0]
    kind, env, opts = SCENARIOS[name]
    out_dir = argv[argv.index("--out") + 1] if "--out" in argv else "."
    os.makedirs(out_dir, exist_ok=True)
    os.environ.update(env)                  # before the library loads: it reads each switch once
    res = (run_train if kind == "train" else run_gen)(opts, out_dir, name)
    res["scenario"] = name
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(res, f)
    print(json.dumps({k: v for k, v in res.items() if k != "tokens"}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
