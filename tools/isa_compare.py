"""Kernel ISA of two source trees, compared per kernel symbol: the proof that a refactor left the compiled kernels alone.
   python tools/isa_compare.py <parent tree> <candidate tree> unit.hip [unit.hip ...] [--parent-units unit.hip ...]
The symbols of all listed units are pooled per tree, so a kernel that moved to another unit is still compared by its
symbol (each line names the unit, `parent unit -> candidate unit` where it moved); --parent-units lists the parent tree's
units where they differ from the candidate's (a unit that did not exist yet). Each unit is compiled in its tree with plbert_amd/build.py's FLAGS and per-source flags (of the tree this script is in)
plus `-x hip --cuda-device-only -S`. Per mangled kernel symbol the instruction lists are compared with directives and
comments dropped and the function number in .LBB<n>_ labels normalised; a function ends at its .Lfunc_end label, so
the symbols and metadata that follow the last one are not taken for code. The resource figures are those of the
.amdgpu_metadata note. One line per symbol, `parent -> candidate` where a figure changed; exit status 1 when a symbol
has a spill, scratch, more VGPRs or another LDS size than in the parent."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from plbert_amd import build as B  # noqa: E402

FIGURES = [("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
           ("vspill", ".vgpr_spill_count"), ("sspill", ".sgpr_spill_count"), ("scratch", ".private_segment_fixed_size")]


def assembly(tree, unit, workdir, tag):
    out = os.path.join(workdir, f"{tag}_{os.path.splitext(unit)[0]}.s")
    cmd = [B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(unit, []), "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(tree, "plbert_amd", "csrc", unit), "-o", out]
    return out, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def kernels(path):
    """{mangled symbol: (instruction list, {figure: value})} of one .s file."""
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text.split(".amdgpu_metadata", 1)[1])[1:]:
        sym = re.search(r"\n    \.name:\s+(\S+)", blk).group(1)
        meta[sym] = {k: int(re.search(r"\n    %s:\s+(\d+)" % re.escape(f), blk).group(1)) for k, f in FIGURES}
    out, cur = {}, None
    for ln in text.splitlines():
        s = ln.split(";")[0].strip()
        if cur is None:
            if s.endswith(":") and s[:-1] in meta:
                cur = out.setdefault(s[:-1], [])
        elif s.startswith(".Lfunc_end"):
            cur = None
        elif s and (not s.startswith(".") or s.startswith(".LBB")):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {sym: (ins, meta[sym]) for sym, ins in out.items()}


def demangle(syms):
    r = subprocess.run(["c++filt"], input="\n".join(syms), text=True, stdout=subprocess.PIPE, check=True).stdout.splitlines()
    short = [re.sub(r"\(anonymous namespace\)::|^void |\(.*\)$", "", d) for d in r]
    return dict(zip(syms, short))


def pooled(tree, units, tmp, tag):
    """{mangled symbol: (unit, instruction list, figures)} over all units of one tree."""
    jobs = [(u, assembly(tree, u, tmp, tag)) for u in units]
    out = {}
    for unit, (path, proc) in jobs:
        o, _ = proc.communicate()
        if proc.returncode:
            raise SystemExit(f"{tag} {unit}:\n{o}")
        for sym, (ins, meta) in kernels(path).items():
            if sym in out:
                raise SystemExit(f"{tag}: {sym} is defined in {out[sym][0]} and in {unit}")
            out[sym] = (unit, ins, meta)
    return out


def main():
    parent, cand, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    punits = units
    if "--parent-units" in units:
        k = units.index("--parent-units")
        units, punits = units[:k], units[k + 1:]
    ver = subprocess.run([B._hipcc(), "--version"], stdout=subprocess.PIPE, text=True).stdout.splitlines()
    print("compiler: " + "; ".join(l.strip() for l in ver if l.startswith(("HIP version", "AMD clang"))))
    bad = n_same = n_diff = 0
    with tempfile.TemporaryDirectory(prefix="isa_compare_") as tmp:
        kp, kc = pooled(parent, punits, tmp, "parent"), pooled(cand, units, tmp, "cand")
    names = demangle(list(kp) + [s for s in kc if s not in kp])
    gone = [f"{kp[s][0]} {names[s]}" for s in kp if s not in kc]
    new = [f"{kc[s][0]} {names[s]}" for s in kc if s not in kp]
    for sym in kp:
        if sym not in kc:
            continue
        (up, lp, mp), (uc, lc, mc) = kp[sym], kc[sym]
        same = lp == lc   # labels included: the same instructions under the same branch targets
        ip, ic = ([i for i in l if not i.endswith(":")] for l in (lp, lc))
        n_same, n_diff = n_same + same, n_diff + (not same)
        fig = lambda a, b, w: f"{a:>{w}}" if a == b else f"{a} -> {b}"  # noqa: E731
        cols = "  ".join(f"{k} {fig(mp[k], mc[k], 6 if k == 'lds' else 3)}" for k, _ in FIGURES)
        print(f"{fig(up, uc, 0):<30} {names[sym]:<62} {fig(len(ip), len(ic), 5)} instructions  {cols}  "
              f"{'identical' if same else 'differs'}")
        if mc["vspill"] or mc["sspill"] or mc["scratch"] or mc["vgpr"] > mp["vgpr"] or mc["lds"] != mp["lds"]:
            bad += 1
    print(f"--- {n_same + n_diff} kernel symbols in both trees: {n_same} identical, {n_diff} differ; "
          f"{len(gone)} only in the parent, {len(new)} only in the candidate; "
          f"{bad} with a spill, scratch, more VGPRs or another LDS size than in the parent")
    for g in gone:
        print("only in the parent:    " + g)
    for n in new:
        print("only in the candidate: " + n)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
