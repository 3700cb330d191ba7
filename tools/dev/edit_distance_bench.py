"""dev: what scoring a decoded test set costs on the device and on the host (the figures of profiles/evaluate.md).

   python tools/dev/edit_distance_bench.py [--pairs 4096] [--reps 1000] [--host_reps 2]

Two length distributions over the project's vocabulary (4,300 ids, specials 0..4), rows 128 columns wide as generate_stream and the
data loader produce them (prediction: [CLS], characters, [SEP], padding; label: characters, padding):
   short   label lengths U{8..60}, the prediction = the label with ~10 % of its characters substituted, dropped or doubled
   long    127 characters on both sides, the same edits
Per distribution:
   kernel  kzv_edit_distance, HIP events around --reps launches that cycle through 4 different input batches (after a warm-up of the
           same launches), distance-only and with every output (ops, both alignment arrays, char_stats); microseconds per launch
   device  the whole device path as kzv.trainer.test runs it -- edit_stats, the three result arrays copied to the host, cer_values --
           wall clock, median of 5, ending on the host with the list of floats
   host    the string path on the same ids: batch_decode x 2 + calculate_cer per line (kzv.model._levenshtein), wall clock
The device and host CER lists are compared (==) before anything is printed."""
import argparse, os, statistics, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.environ.get("KZV_PKG") or os.path.join(ROOT, "kuzushiji-vision_amd"))
import ctypes as C
import numpy as np
import torch
from kzv import _lib as L
from kzv import metrics as M
from kzv.config import vit_b_config
from kzv.data import build_decoder_dir
from kzv.model import TrOCRModel

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=4096)
ap.add_argument("--reps", type=int, default=1000)
ap.add_argument("--host_reps", type=int, default=2)
a = ap.parse_args()

cfg = vit_b_config()
V, W, PAD, BOS, EOS = cfg.vocab, 128, cfg.pad_id, cfg.bos_id, cfg.eos_id
with tempfile.TemporaryDirectory() as tmp:
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(build_decoder_dir(os.path.join(tmp, "d"), cfg))
assert M.is_one_char_tokenizer(tok)
special = tok.all_special_ids
lib = L.load()


def batch(lengths, seed):
    rng = np.random.default_rng(seed)
    ref = np.full((a.pairs, W), PAD, dtype=np.int64)
    pred = np.full((a.pairs, W), PAD, dtype=np.int64)
    for k in range(a.pairs):
        r = rng.integers(5, V, int(lengths(rng)))
        u = rng.random(r.size)
        p = []
        for t, x in zip(r.tolist(), u.tolist()):
            if x < 0.033:
                continue
            p.append(int(rng.integers(5, V)) if x < 0.066 else t)
            if x > 0.967:
                p.append(t)
        p = [BOS] + p[:W - 2] + [EOS]
        ref[k, :r.size] = r
        pred[k, :len(p)] = p[:W]
    return torch.from_numpy(pred).cuda(), torch.from_numpy(ref).cuda()


def events(fn, sets):
    for s in sets:
        fn(*s)                                               # warm-up: the same launches
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(a.reps):
        fn(*sets[i % len(sets)])
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.reps


print(f"{a.pairs} pairs, vocabulary {V}, rows of {W} columns; {a.reps} launches per event pair over 4 input batches")
print("| lengths | mean CER | kernel, distance only (us) | kernel, all outputs (us) | device path to host floats (ms) | host string path (ms) | host / device |")
print("|---|---|---|---|---|---|---|")
for name, lengths in (("U{8..60}", lambda rng: rng.integers(8, 61)), ("127 / 127", lambda rng: 127)):
    sets = [batch(lengths, seed) for seed in (11, 12, 13, 14)]
    table = torch.zeros(V, 5, dtype=torch.int32, device="cuda")
    out = [torch.empty(a.pairs, dtype=torch.int32, device="cuda") for _ in range(3)]
    ops = torch.empty(a.pairs, 4, dtype=torch.int32, device="cuda")
    maps = [torch.empty(a.pairs, W, dtype=torch.int32, device="cuda") for _ in range(2)]

    def raw(full):                                           # the C call alone, on outputs allocated once
        def fn(p, r):
            arg = L.kzv_edit_args(pred=p.data_ptr(), ld_pred=W, ref=r.data_ptr(), ld_ref=W, n=a.pairs, width_pred=W, width_ref=W, vocab=V,
                                  n_special=len(special), special=(C.c_int32 * 8)(*special), dist=out[0].data_ptr(), ref_len=out[1].data_ptr(),
                                  pred_len=out[2].data_ptr(), ops=ops.data_ptr() if full else None, ref_to_pred=maps[0].data_ptr() if full else None,
                                  pred_to_ref=maps[1].data_ptr() if full else None, ld_align=W, char_stats=table.data_ptr() if full else None)
            L.check(lib.kzv_edit_distance(C.byref(arg), L.stream_handle()), "kzv_edit_distance")
        return fn

    t_dist = events(raw(False), sets)
    t_full = events(raw(True), sets)

    def device_path(p, r):
        st = M.edit_stats(p, r, special, V, ops=False)
        return M.cer_values(st["dist"], st["ref_len"], st["pred_len"])

    dev_ms = []
    for i in range(6):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        cer_dev = device_path(*sets[i % 4])
        if i:
            dev_ms.append((time.perf_counter() - t0) * 1e3)
    pred, ref = sets[5 % 4]
    host_ms = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        ps = tok.batch_decode(pred, skip_special_tokens=True)
        ts = tok.batch_decode(ref, skip_special_tokens=True)
        cer_host = [TrOCRModel.calculate_cer(None, x, y) for x, y in zip(ps, ts)]
        host_ms.append((time.perf_counter() - t0) * 1e3)
    assert cer_dev == cer_host, "device and host CER differ"
    d, h = statistics.median(dev_ms), statistics.median(host_ms)
    print(f"| {name} | {sum(cer_host) / len(cer_host):.4f} | {t_dist:.1f} | {t_full:.1f} | {d:.2f} (spread {max(dev_ms) - min(dev_ms):.2f}) | "
          f"{h:.0f} (spread {max(host_ms) - min(host_ms):.0f}) | {h / d:.0f} |", flush=True)
