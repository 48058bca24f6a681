"""Device-code equality of two trees, kernel by kernel: the rule for refactors of the
hand-scheduled kernels (DESIGN.md "Refactoring the step kernels").

  python tools/listing_diff.py THIS OTHER [--defines "" PBN_STAMPS PBN_CHECKS]
                               [--sources pbn_env.hip isa:pipe ...] [--cache DIR] [--jobs N]

THIS is a checkout; OTHER is a checkout too, or, if it is no directory, a git revision of THIS,
exported into a temporary directory.  Every source of pbn_rl_amd._lib.SOURCES is compiled to a
gfx950 assembly listing (the product's flags, --offload-device-only -S) once per entry of
--defines (the empty string is the product build), and the two single-kernel instances of
tools/isa_budget.py (isa:pipe, isa:settle) with its -DPBN_ISA_MARKS.  A listing is cut at its
symbols; what is compared per symbol is all of its text: the instruction stream, the
.amdhsa_kernel block (registers, scratch, LDS) and the compiler's resource comments, and the
symbol's entry of the code object's metadata.  The function index in local labels is
normalised, so kernels may change their order in the file; the lines naming the compilation
unit's id (a hash of the source's path) are dropped.  Prints one line per symbol that differs,
is missing or is new, and exits non-zero if there is one.

--cache DIR keeps listings by a hash of (csrc/, include/, the source, the defines), so that an
unchanged tree -- the parent, typically -- is compiled once over many runs.
"""
import argparse
import concurrent.futures
import difflib
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

import isa_budget  # noqa: E402
from pbn_rl_amd._lib import SOURCES  # noqa: E402

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"]   # _lib.build's
ISA_INSTANCES = {"isa:" + k: v[0] % {"W": 1, "B": 16} for k, v in isa_budget.KERNELS.items()}
CONFIGS = ["", "PBN_STAMPS", "PBN_CHECKS"]


def tree_hash(root):
    h = hashlib.sha256()
    for sub in ("pbn_rl_amd/csrc", "include"):
        for name in sorted(os.listdir(os.path.join(root, sub))):
            path = os.path.join(root, sub, name)
            if os.path.isfile(path):
                h.update(name.encode() + b"\0" + open(path, "rb").read() + b"\0")
    return h.hexdigest()[:24]


def compile_listing(root, source, defines, out_s):
    if source in ISA_INSTANCES:
        isa_budget.compile_listing(ISA_INSTANCES[source], out_s, root=root)
        return
    src = os.path.join(root, "pbn_rl_amd", "csrc", source)
    subprocess.run(["hipcc", *FLAGS, *["-D" + d for d in defines.split(",") if d], "--offload-device-only",
                    "-S", src, "-o", out_s], check=True, cwd=os.path.dirname(src), stderr=subprocess.DEVNULL)


def listing(root, source, defines, cache, tmp):
    """The text of one listing, compiled or taken from the cache."""
    tag = "%s_%s_%s.s" % (tree_hash(root), source.replace(":", "_"), defines.replace(",", "+") or "product")
    path = os.path.join(cache or tmp, tag)
    if not os.path.exists(path):
        fd, part = tempfile.mkstemp(dir=os.path.dirname(path), suffix=".part")
        os.close(fd)
        compile_listing(root, source, defines, part)
        os.replace(part, path)
    with open(path) as f:
        return f.read()


LOCAL = re.compile(r"\.L(BB|func_begin|func_end|JTI|tmp|CPI)\d+")
HEAD = re.compile(r"^\s*\.(globl|protected|weak|hidden|p2align|section|text)\b")
TYPE = re.compile(r"^\s*\.type\s+([^,\s]+),@(function|object)")


def symbols(text):
    """{symbol: [lines]} of a listing; "" is what precedes the first symbol, "meta:<symbol>" a
    kernel's entry of the metadata."""
    lines = [LOCAL.sub(lambda m: ".L" + m.group(1), ln.rstrip()) for ln in text.splitlines()
             if "__hip_cuid_" not in ln]
    meta_at = next((i for i, ln in enumerate(lines) if ln.strip() == ".amdgpu_metadata"), len(lines))
    out, name, cur = {}, "", []
    for i, ln in enumerate(lines[:meta_at]):
        m = TYPE.match(ln)
        if m:
            k = len(cur)
            while k and HEAD.match(cur[k - 1]):   # the directives that introduce the symbol
                k -= 1
            out.setdefault(name, []).extend(cur[:k])
            name, cur = m.group(1), cur[k:]
        cur.append(ln)
    out.setdefault(name, []).extend(cur)
    item, key = [], None   # a kernel's entry: from its "  - " line to the next one or to a top-level key
    for ln in lines[meta_at:] + [""]:
        if ln.startswith("  - ") or not ln.startswith(" "):
            if item:
                out["meta:" + (key or "")] = item
            item, key = [], None
        if not ln.startswith(" "):   # directives, top-level keys, the document's ends
            out.setdefault("meta", []).append(ln)
            continue
        m = re.match(r"^\s+\.symbol:\s+'?([^'\s]+?)(\.kd)?'?$", ln)
        if m:
            key = m.group(1)
        item.append(ln)
    return out


def compare(a_text, b_text, show):
    """Lines of report for one pair of listings."""
    a, b = symbols(a_text), symbols(b_text)
    report = []
    for sym in sorted(set(a) | set(b)):
        if sym not in b:
            report.append("only in THIS   %s" % sym)
        elif sym not in a:
            report.append("only in OTHER  %s" % sym)
        elif a[sym] != b[sym]:
            d = [x for x in difflib.unified_diff(b[sym], a[sym], "OTHER", "THIS", lineterm="", n=0)][2:]
            n = sum(1 for x in d if x[0] in "+-")
            report.append("differs        %s  (%d lines)" % (sym or "<file head>", n) +
                          "".join("\n      " + x for x in d[:show]))
    return report, len(a)


def export(repo, rev, dest):
    os.makedirs(dest)
    tar = subprocess.run(["git", "-C", repo, "archive", rev, "pbn_rl_amd/csrc", "include"], check=True,
                         stdout=subprocess.PIPE).stdout
    subprocess.run(["tar", "-x", "-C", dest], input=tar, check=True)
    return dest


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("this")
    ap.add_argument("other", help="a checkout, or a git revision of THIS")
    ap.add_argument("--defines", nargs="*", default=CONFIGS,
                    help="one build per entry, comma-separated names; \"\" is the product build")
    ap.add_argument("--sources", nargs="*", default=SOURCES + sorted(ISA_INSTANCES))
    ap.add_argument("--cache", default=None, help="keep listings here between runs")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--show", type=int, default=0, help="print this many diff lines per symbol")
    a = ap.parse_args()
    t0 = time.time()
    tmp = tempfile.mkdtemp(prefix="listing_diff_")
    try:
        if not os.path.isdir(a.this):
            ap.error("THIS must be a checkout (a directory): %s" % a.this)
        roots = [os.path.abspath(a.this), os.path.abspath(a.other) if os.path.isdir(a.other)
                 else export(a.this, a.other, os.path.join(tmp, "rev"))]
        if a.cache:
            os.makedirs(a.cache, exist_ok=True)
        pairs = [(s, "PBN_ISA_MARKS" if s in ISA_INSTANCES else d) for s in a.sources
                 for d in (a.defines if s not in ISA_INSTANCES else [""])]
        bad = 0
        with concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
            jobs = {(s, d): [pool.submit(listing, r, s, "" if s in ISA_INSTANCES else d, a.cache, tmp)
                             for r in roots] for s, d in pairs}
            for (s, d), (fa, fb) in jobs.items():
                report, n = compare(fa.result(), fb.result(), a.show)
                print("%-16s %-14s %4d symbols, %d differ" % (s, d or "product", n, len(report)), flush=True)
                for ln in report:
                    print("  " + ln)
                bad += len(report)
        print("%d symbols differ; %.0f s" % (bad, time.time() - t0))
        return 1 if bad else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
