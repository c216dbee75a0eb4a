"""Compare the decode kernels' and the two writers' device code between two source trees, kernel
by kernel:
    python tools/isa_diff.py OLD_TREE NEW_TREE [--diag] [-DFLAG ...]
Each tree's kernel translation units (whichever of KERNEL_TUS it has) are compiled to gfx950
assembly and every kernel's instruction stream is compared after dropping comments and assembler
directives and the function index in its `.LBB<n>_<m>` labels (it only counts the functions in
front of it in the file).  Prints `same` or `DIFF` per kernel and exits nonzero on any DIFF or
unmatched kernel.  --diag compares the diagnostic library's build (-DGPD_DIAG).
A refactor of the kernels' sources is checked with this on the CPU before any GPU run: the
register allocator's choices move between near-identical sources (tools/isa_count.py)."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CXXFILT = os.environ.get("CXXFILT", "c++filt")
KERNEL_TUS = ["gpd_kernels.hip", "gpd_rs.hip", "gpd_ro.hip", "gpd_sp.hip", "gpd_pcapwrite.hip",
              "gpd_pcapngwrite.hip"]


def kernel_tus(tree):
    csrc = os.path.join(tree, "gopacket_amd", "csrc")
    return [os.path.join(csrc, f) for f in KERNEL_TUS if os.path.exists(os.path.join(csrc, f))]


def compile_tree(tree, flags, tmp, tag):
    """{mangled kernel name: [normalised instruction lines]} over the tree's kernel TUs."""
    srcs = kernel_tus(tree)
    outs = [os.path.join(tmp, f"{tag}_{os.path.basename(s)}.s") for s in srcs]
    cmds = [[HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(tree, "include"), *flags,
             "-S", "--cuda-device-only", s, "-o", o] for s, o in zip(srcs, outs)]
    with ThreadPoolExecutor(max_workers=len(cmds)) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), cmds):
            if r.returncode != 0:
                sys.exit(r.stderr)
    kernels = {}
    for o in outs:
        txt = open(o).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M):
            start = txt.index("\n" + name + ":") + len(name) + 2
            body = txt[start:txt.index(".Lfunc_end", start)]
            kernels[name] = normalise(body)
    return kernels


def normalise(body):
    lines = []
    for l in body.splitlines():
        l = l.split(";", 1)[0].strip()
        if not l or (l.startswith(".") and not l.endswith(":")):
            continue  # comment or directive (labels stay)
        lines.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
    return lines


def key(demangled):
    """A kernel's identity across the trees: its demangled name, or for decode_kernel its
    (STAGE, EXT, PAGES) — the older form carries retired template arguments."""
    m = re.match(r"(?:void )?gpd::decode_kernel<(.*)>\(", demangled)
    if m:
        a = [x.strip() for x in m.group(1).split(",")]
        stage, ext, pages = (a[0], a[2], a[3]) if len(a) == 9 else a
        return f"gpd::decode_kernel<STAGE={stage}, EXT={ext}, PAGES={pages}>"
    return re.sub(r"^void ", "", demangled.replace("(anonymous namespace)::", "")).split("(")[0]


def keyed(kernels):
    names = sorted(kernels)
    dem = subprocess.run([CXXFILT], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {key(d): kernels[n] for n, d in zip(names, dem)}


def main():
    trees = [a for a in sys.argv[1:] if not a.startswith("-")]
    if len(trees) != 2:
        sys.exit(__doc__)
    flags = [a for a in sys.argv[1:] if a.startswith("-D")] + (["-DGPD_DIAG"] if "--diag" in sys.argv else [])
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=2) as ex:
        old, new = ex.map(lambda t: keyed(compile_tree(t[0], flags, tmp, t[1])), zip(trees, ("old", "new")))
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            verdict = "only in " + ("OLD" if k in old else "NEW")
        else:
            verdict = "same" if old[k] == new[k] else "DIFF"
        bad += verdict != "same"
        n = len(new.get(k, old.get(k)))
        print(f"{verdict:12s} {n:6d} lines  {k}")
    print(f"{len(set(old) | set(new))} kernels, {bad} not the same" + (" (diag build)" if "--diag" in sys.argv else ""))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
