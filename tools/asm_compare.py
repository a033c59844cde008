"""Compare the gfx950 device assembly of csrc translation units between two source trees, kernel by kernel.

    python tools/asm_compare.py --base <tree or git revision> [--head <tree>] [--keep DIR] [--kernels] unit.hip ...

Each unit is compiled in both trees with build.py's flags and that unit's extra flags, for the device only, to assembly.
Comments, the .file / .loc / .ident lines and the __hip_cuid_ symbol (a hash that every compilation makes anew) are dropped; what is left is compared as text, and nothing else is looked at.
One row per unit: instruction-line count (base, head), "same" when the whole text is equal, and the kernels that differ.
With --kernels one row per kernel too: instruction lines and the VGPR / AGPR / SGPR / LDS / scratch / spill figures of the
kernel's metadata, base and head.  A git revision is exported to a temporary tree.  Nothing is linked or run.
"""
import argparse
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from points_matching_amd import build as B  # noqa: E402

FIGURES = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
           ("scratch", ".private_segment_fixed_size"), ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count"))


def export(rev, where):
    os.makedirs(where, exist_ok=True)
    tar = os.path.join(where, "base.tar")
    subprocess.run(["git", "-C", ROOT, "archive", "-o", tar, rev, "points_matching_amd/csrc", "include"], check=True)
    with tarfile.open(tar) as t:
        t.extractall(where)
    os.remove(tar)
    return where


def assembly(tree, unit, keep):
    csrc = os.path.join(tree, "points_matching_amd", "csrc")
    flags = [f for f in B.FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"), "-I" + csrc, "-I/opt/rocm/include"]
    extra = [f for f in B.EXTRA.get(unit, []) if not f.startswith("-Rpass")]
    out = os.path.join(keep, unit.rsplit(".", 1)[0] + ".s")
    cmd = [B.HIPCC] + flags + extra + ["-x", "hip", "--offload-device-only", "-S", os.path.join(csrc, unit), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("%s\n%s" % (" ".join(cmd), r.stderr))
    with open(out) as f:
        return strip(f.read())


def strip(text):
    lines = []
    for ln in text.splitlines():
        ln = ln.split(";", 1)[0].rstrip()
        if not ln.strip() or re.match(r"\s*\.(file|loc|ident)\b", ln) or "__hip_cuid_" in ln:
            continue
        lines.append(ln)
    return lines


def kernels(lines):
    """name -> (body lines, descriptor lines, metadata figures); plus the instruction-line count of the unit."""
    body, desc, meta = {}, {}, {}
    cur = None
    for i, ln in enumerate(lines):
        m = re.match(r"(\w+):$", ln)
        if m and i and lines[i - 1].strip().startswith((".type", ".p2align", ".globl", ".weak", ".protected")):
            cur = m.group(1)
            body[cur] = []
        elif re.match(r"\.Lfunc_end\d+:", ln):
            cur = None
        elif cur:
            body[cur].append(ln)
    cur = None
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            cur = m.group(1)
            desc[cur] = []
        elif ln.strip() == ".end_amdhsa_kernel":
            cur = None
        elif cur:
            desc[cur].append(ln.strip())
    block = []
    for ln in lines + ["  - .end"]:
        s = ln.strip()
        if s.startswith("- .") and block:
            d = dict(b.lstrip("- ").split(":", 1) for b in block if ":" in b)
            if ".name" in d and ".vgpr_count" in d:
                meta[d[".name"].strip()] = {k: d.get(key, "0").strip() for k, key in FIGURES}
            block = []
        if s.startswith((".", "- .")):
            block.append(s)
    return body, desc, meta


def count(body):
    return sum(1 for ln in body if ln.startswith(("\t", " ")) and not ln.strip().startswith("."))


def demangle(name):
    d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    d = re.sub(r"(\w+::)?\(anonymous namespace\)::", "", d)
    return re.sub(r"^void ", "", re.sub(r"\((?!.*>).*$", "", d))[:70]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base", required=True)
    ap.add_argument("--head", default=ROOT)
    ap.add_argument("--keep", default=None, help="directory that keeps the .s files (base/ and head/ below it)")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("units", nargs="+")
    a = ap.parse_args()
    tmp = tempfile.TemporaryDirectory()
    base = a.base if os.path.isdir(a.base) else export(a.base, os.path.join(tmp.name, "tree"))
    keep = a.keep or os.path.join(tmp.name, "asm")
    for side in ("base", "head"):
        os.makedirs(os.path.join(keep, side), exist_ok=True)
    jobs = [(t, u, os.path.join(keep, s)) for u in a.units for s, t in (("base", base), ("head", a.head))]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        texts = list(ex.map(lambda j: assembly(*j), jobs))
    print("| unit | lines base | lines head | same | kernels that differ |")
    print("|---|---|---|---|---|")
    detail = []
    status = 0
    for i, unit in enumerate(a.units):
        tb, th = texts[2 * i], texts[2 * i + 1]
        (bb, db, mb), (bh, dh, mh) = kernels(tb), kernels(th)
        differ = [k for k in sorted(set(bb) | set(bh)) if bb.get(k) != bh.get(k) or db.get(k) != dh.get(k) or mb.get(k) != mh.get(k)]
        same = tb == th
        status |= 0 if same else 1
        print("| %s | %d | %d | %s | %s |" % (unit.rsplit(".", 1)[0], count(tb), count(th), "yes" if same else "no",
                                            ", ".join(demangle(k) for k in differ) or ("-" if same else "(outside kernels)")))
        for k in sorted(set(mb) | set(mh)):
            if a.kernels or k in differ:
                fb, fh = mb.get(k, {}), mh.get(k, {})
                detail.append("| %s | %s | %s | %d / %d | %s |" % (
                    unit.rsplit(".", 1)[0], demangle(k), "yes" if k not in differ else "no", count(bb.get(k, [])), count(bh.get(k, [])),
                    " ".join("%s %s/%s" % (n, fb.get(n, "-"), fh.get(n, "-")) for n, _ in FIGURES)))
    if detail:
        print("\n| unit | kernel | same | instruction lines base / head | figures base/head |")
        print("|---|---|---|---|---|")
        print("\n".join(detail))
    return status


if __name__ == "__main__":
    sys.exit(main())
