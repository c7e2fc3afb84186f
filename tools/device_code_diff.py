"""Compare the gfx950 device code of two source trees, translation unit by translation unit.

    python tools/device_code_diff.py TREE_A TREE_B [--work DIR] [--only NAME,...] [--jobs N] [--report FILE]

Every job of each tree's zest-nerf_amd/build_hip.py (the fused variants and the sources, each with that job's own
flags) is compiled device-only to assembly, on the command line build_hip._compile uses with `-c` replaced by
`--cuda-device-only -S`.  Lines that cannot be code are dropped (.file, .ident, comment lines) and the one thing hipcc
derives from the path of the source is normalised (the compilation-unit id in `__hip_cuid_<hash>`); what is left is
hashed and compared.  For every kernel the .amdhsa resource fields are listed: VGPRs, SGPRs, scratch, LDS bytes.
The tool hashes and diffs only; it looks for no particular instruction.  The digests change with the compiler,
so a report is a record of one comparison, not something to pin in a test.

Assembly is kept in --work (default: a temporary directory) and reused while it is newer than the tree's sources.
"""
import argparse
import difflib
import hashlib
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

MAX_JOBS = 16
FIELDS = [("vgpr", ".amdhsa_next_free_vgpr"), ("sgpr", ".amdhsa_next_free_sgpr"),
          ("scratch", ".amdhsa_private_segment_fixed_size"), ("lds", ".amdhsa_group_segment_fixed_size")]
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def load_build(tree):
    path = os.path.join(tree, "zest-nerf_amd", "build_hip.py")
    spec = importlib.util.spec_from_file_location("build_hip_" + hashlib.md5(path.encode()).hexdigest(), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def jobs_of(b):
    every = [(name, "fused_variant.hip", flags) for name, flags in b.VARIANTS]
    every += [(s.replace(".hip", ""), s, b.SOURCE_FLAGS.get(s, [])) for s in b.SOURCES]
    return every


def newest_source(b):
    files = [os.path.join(b.CSRC, f) for f in os.listdir(b.CSRC) if f.endswith((".hip", ".cuh", ".h"))]
    files += [os.path.join(b.HERE, "build_hip.py"), os.path.join(b.HERE, "..", "include", "zest_render.h")]
    return max(os.path.getmtime(f) for f in files)


def compile_asm(b, job, outdir, newest):
    name, src, flags = job
    out = os.path.join(outdir, name + ".s")
    if not (os.path.exists(out) and os.path.getmtime(out) > newest):
        cmd = [b.HIPCC] + b.FLAGS + flags + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-S",
                                             os.path.join(b.CSRC, src), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s (%s):\n%s" % (name, b.CSRC, r.stderr[-6000:]))
    return out


def code_lines(path):
    keep = []
    with open(path) as f:
        for line in f:
            s = line.strip()
            if not s or s.startswith((";", "//", ".file", ".ident")):
                continue
            keep.append(CUID.sub("__hip_cuid_X", line.rstrip()))
    return keep


def resources(lines):
    """{kernel: {field: value}} from the .amdhsa_kernel blocks"""
    res, cur = {}, None
    for line in lines:
        t = line.split()
        if t[0] == ".amdhsa_kernel":
            cur = res.setdefault(t[1], {})
        elif t[0] == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None:
            for key, directive in FIELDS:
                if t[0] == directive:
                    cur[key] = t[1]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--work", help="directory for the assembly (kept); default: a temporary one")
    ap.add_argument("--only", help="comma-separated job names (fused_bf16_s0, volume_cost, ...)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--report", help="also write the report to this file")
    ap.add_argument("--label-a", default="A")
    ap.add_argument("--label-b", default="B")
    args = ap.parse_args()
    tmp = None if args.work else tempfile.TemporaryDirectory()
    work = args.work or tmp.name
    only = args.only.split(",") if args.only else None

    trees = []
    for side, tree in (("a", args.tree_a), ("b", args.tree_b)):
        b = load_build(os.path.abspath(tree))
        outdir = os.path.join(work, side)
        os.makedirs(outdir, exist_ok=True)
        trees.append((b, [j for j in jobs_of(b) if not only or j[0] in only], outdir, newest_source(b)))
    names_a, names_b = [j[0] for j in trees[0][1]], [j[0] for j in trees[1][1]]
    if names_a != names_b:
        sys.exit("the two trees do not build the same jobs: %s" % sorted(set(names_a) ^ set(names_b)))
    with ThreadPoolExecutor(max_workers=max(1, min(args.jobs, MAX_JOBS))) as ex:
        futs = [[ex.submit(compile_asm, b, j, outdir, newest) for j in jobs] for b, jobs, outdir, newest in trees]
        asm = [[f.result() for f in side] for side in futs]

    b0 = trees[0][0]
    version = subprocess.run([b0.HIPCC, "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    out = ["device code identity: %s against %s" % (args.label_a, args.label_b),
           "compiler: " + " | ".join(l.strip() for l in version[:2]),
           "flags: " + " ".join(b0.FLAGS) + " + each job's own, --cuda-device-only -S",
           "compared: assembly without .file / .ident / comment lines, __hip_cuid_<hash> normalised", ""]
    table, diffs, n_same, n_kernels, n_kernels_same = [], [], 0, 0, 0
    out.append("%-22s %-10s %-16s %-16s" % ("translation unit", "verdict", "sha256 " + args.label_a, "sha256 " + args.label_b))
    for name, pa, pb in zip(names_a, asm[0], asm[1]):
        la, lb = code_lines(pa), code_lines(pb)
        ha, hb = (hashlib.sha256("\n".join(l).encode()).hexdigest()[:16] for l in (la, lb))
        same = la == lb
        n_same += same
        out.append("%-22s %-10s %-16s %-16s" % (name, "identical" if same else "DIFFERENT", ha, hb))
        if not same:
            d = list(difflib.unified_diff(la, lb, args.label_a + "/" + name, args.label_b + "/" + name, lineterm="", n=2))
            diffs += d[:60] + (["... (%d more diff lines)" % (len(d) - 60)] if len(d) > 60 else []) + [""]
        ra, rb = resources(la), resources(lb)
        for k in sorted(set(ra) | set(rb)):
            va, vb = ra.get(k), rb.get(k)
            n_kernels += 1
            n_kernels_same += va == vb
            row = [(va or {}).get(key, "-") if va == vb else "%s>%s" % ((va or {}).get(key, "-"), (vb or {}).get(key, "-"))
                   for key, _ in FIELDS]
            table.append("%-22s %5s %5s %8s %7s  %-5s %s" % (name, *row, "same" if va == vb else "DIFF", k))
    out += ["", "%d of %d translation units identical; %d of %d kernels with identical resource fields"
            % (n_same, len(names_a), n_kernels_same, n_kernels), "",
            "%-22s %5s %5s %8s %7s  %-5s %s" % ("translation unit", "vgpr", "sgpr", "scratch", "lds", "", "kernel")] + table
    if diffs:
        out += ["", "first differences:"] + diffs
    text = "\n".join(out) + "\n"
    sys.stdout.write(text)
    if args.report:
        with open(args.report, "w") as f:
            f.write(text)
    return 0 if n_same == len(names_a) and n_kernels_same == n_kernels else 1


if __name__ == "__main__":
    sys.exit(main())
