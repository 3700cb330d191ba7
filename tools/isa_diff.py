"""Proof that a source change left kernels alone: compiles the same .hip units of two trees with the Makefile's flags (its per-unit overrides included: UNIT_FLAGS) and compares
the gfx950 assembly kernel by kernel.
   python tools/isa_diff.py PARENT_CSRC [--new CSRC] [--units attention.hip gemm_nt256p.hip ...] [--cache DIR] [--show] [--strict]
                            [--rename REGEX REPLACEMENT] [--parent-units decode.hip ...]
(--parent-units: a unit was split, merged or renamed: the kernels of those PARENT units, pooled, are matched by demangled name against
the pooled kernels of --units; --rename rewrites the parent's demangled kernel names before they are matched, for a kernel template that gained a parameter:
--rename 'decode_fused_kernel<(\d)>' 'decode_fused_kernel<\1, 1>'; --units takes any .hip units of csrc, default: csrc/attention*.hip; --cache keeps the parent's assembly between runs; --show prints
the diff of every kernel whose instruction stream differs).  Per kernel it reports
   (a) the resource counts (.vgpr_count, .agpr_count, .sgpr_count, LDS, scratch, spills: equal to the parent's; a count of
       scratch or spills that is not 0 is noted on the kernel's line) and the MULTISET of instructions, an
       instruction being its mnemonic plus its cache-policy modifiers (nt, sc0, sc1): registers, immediates, labels ignored;
   (b) whether the instruction STREAM is identical line for line (comments, directives and symbol names stripped).
Exit code 1 if (a) fails for any kernel, or a kernel exists on one side only; with --strict also if (b) is not "identical" for any
kernel (the proof a pure refactor owes: the code objects did not move at all)."""
import argparse, collections, difflib, glob, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kuzushiji-vision_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-ffp-contract=fast"]   # csrc/Makefile
UNIT_FLAGS = {"lm_fusion.hip": ["-ffp-contract=off"]}      # csrc/Makefile's per-unit rules (build/lm_fusion.o: FLAGS += ...): appended, the last one wins
META = [".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size", ".vgpr_spill_count", ".sgpr_spill_count"]


def asm_of(unit, out):      # "<stem>-hip-amdgcn-amd-amdhsa-gfx950.s": the whole stem, so that gemm.hip does not pick up gemm_rows.hip's
    return glob.glob(os.path.join(out, os.path.splitext(unit)[0] + "-hip-*gfx950.s"))


def compile_unit(csrc, unit, out):
    os.makedirs(out, exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *UNIT_FLAGS.get(unit, []), "--save-temps=obj", "-c", unit, "-o", os.path.join(out, unit + ".o")], check=True, cwd=csrc)
    return asm_of(unit, out)[0]


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$", "", d) for d in r.stdout.splitlines()]


def parse(asm):
    """{demangled kernel: (meta dict, [normalised instruction lines])}"""
    text = open(asm, encoding="utf-8", errors="replace").read()
    meta = {}
    for entry in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])[1:]:
        f = dict(re.findall(r"^\s*(\.\w+):\s*(\S+)\s*$", entry, re.M))
        if ".name" in f:
            meta[f[".name"].strip("'\"")] = {k: f.get(k, "?") for k in META}
    body, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1) if m.group(1) in meta else None
            if cur:
                body[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        t = line.split(";")[0].strip()
        if cur is None or not t or (t.startswith(".") and not t.endswith(":")):
            continue
        body[cur].append(re.sub(r"\s+", " ", re.sub(r"_Z\w+", "SYM", t)))
    for n, lines in body.items():      # labels renumbered in order of appearance: a helper more or less renumbers the compiler's
        order = {}
        for t in lines:
            if t.endswith(":"):
                order.setdefault(t[:-1], f".L{len(order)}")
        body[n] = [re.sub(r"\.LBB\d+_\d+", lambda m: order.get(m.group(0), m.group(0)), t) for t in lines]
    names = sorted(body)
    return {d: (meta[n], body[n]) for n, d in zip(names, demangle(names))}


def key(ins):      # mnemonic + cache-policy modifiers (a label counts as a label, whatever its number)
    w = ins.split()
    if w[0].endswith(":"):
        return "label:"
    return " ".join([w[0]] + sorted(x for x in w[1:] if x in ("nt", "sc0", "sc1")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("--new", default=CSRC)
    ap.add_argument("--units", nargs="*")
    ap.add_argument("--parent-units", nargs="+")
    ap.add_argument("--cache")
    ap.add_argument("--show", action="store_true")
    ap.add_argument("--strict", action="store_true")
    ap.add_argument("--rename", nargs=2, metavar=("REGEX", "REPLACEMENT"))
    a = ap.parse_args()
    units = a.units or sorted(os.path.basename(f) for f in glob.glob(os.path.join(a.new, "attention*.hip")))
    with tempfile.TemporaryDirectory() as tmp:
        pdir = a.cache or os.path.join(tmp, "parent")

        def parent_asm(u):
            hit = asm_of(u, pdir)
            return hit[0] if hit else compile_unit(os.path.abspath(a.parent), u, pdir)
        with ThreadPoolExecutor(8) as ex:
            old = list(ex.map(parent_asm, a.parent_units or units))
            new = list(ex.map(lambda u: compile_unit(os.path.abspath(a.new), u, os.path.join(tmp, "new")), units))

        def pooled(files):
            out = {}
            for f in files:
                out.update(parse(f))
            return out
        # one comparison per unit; with --parent-units one comparison of the two pools
        pairs = [("+".join(units), pooled(old), pooled(new))] if a.parent_units else [(u, parse(fo), parse(fn)) for u, fo, fn in zip(units, old, new)]
        bad = 0
        for u, ko, kn in pairs:
            if a.rename:
                ko = {re.sub(a.rename[0], a.rename[1], k): v for k, v in ko.items()}
            for name in sorted(set(ko) | set(kn)):
                if name not in ko or name not in kn:
                    print(f"{u}: {name}: only in {'parent' if name in ko else 'new'}")
                    bad += 1
                    continue
                (mo, bo), (mn, bn) = ko[name], kn[name]
                a_ok = mo == mn and collections.Counter(map(key, bo)) == collections.Counter(map(key, bn))
                spills = [k for k in META[4:] if mn[k] != "0"]
                bad += not a_ok or (a.strict and bo != bn)
                print(f"{u}: {name}: vgpr {mn['.vgpr_count']} agpr {mn['.agpr_count']} sgpr {mn['.sgpr_count']} lds {mn['.group_segment_fixed_size']} "
                      f"instructions {len(bn)}  (a) {'ok' if a_ok else 'FAIL'}  (b) {'identical' if bo == bn else 'DIFFERS'}"
                      + "".join(f"  NOTE {k} {mn[k]} (parent {mo[k]})" for k in spills))
                if not a_ok:
                    print("   parent:", mo, len(bo), "\n   new:   ", mn, len(bn))
                    d = collections.Counter(map(key, bn))
                    d.subtract(collections.Counter(map(key, bo)))
                    print("   multiset (new - parent):", {k: v for k, v in d.items() if v})
                if bo != bn and a.show:
                    print("\n".join("   " + x for x in difflib.unified_diff(bo, bn, "parent", "new", n=2, lineterm="")))
        print(f"{len(units)} units: {bad} kernels failed" + (" (strict)" if a.strict else ""))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
