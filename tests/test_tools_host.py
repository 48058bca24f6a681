"""Host logic of the profile summaries (no GPU): the launches that carry the hand-off's own-shard
copy (pbn_rollout_copy: the pipelined kernel at 256 threads per block) and the standalone copy
kernel stay out of the rollout kernel's averages, and the hand-off trace is cut into reps."""
import csv
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPE = "void (anonymous namespace)::pbn_rollout_pipe<1, 16, false>((anonymous namespace)::StepArgs)"


def _write(path, header, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        w.writerows(rows)


def test_pmc_summary_leaves_out_copy_launches(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import pmc_summary
    finally:
        sys.path.pop(0)
    hdr = ["Kernel_Name", "Workgroup_Size", "Counter_Name", "Counter_Value"]
    rows = [[PIPE, "192", "WRITE_SIZE", "100"], [PIPE, "192", "WRITE_SIZE", "110"],
            [PIPE, "256", "WRITE_SIZE", "300"], ["pbn_copy_kernel", "256", "WRITE_SIZE", "900"]]
    p = str(tmp_path / "c.csv")
    _write(p, hdr, rows)
    mean, n, name = pmc_summary.mean_counter(p, "WRITE_SIZE", "pbn_rollout_pipe")
    assert (mean, n, name) == (105.0, 2, PIPE)


def test_kernel_trace_summary_leaves_out_copy_launches(tmp_path):
    hdr = ["Kernel_Name", "Workgroup_Size_X", "Start_Timestamp", "End_Timestamp"]
    rows = [[PIPE, "192", "0", "20000"], [PIPE, "192", "100000", "124000"], [PIPE, "256", "200000", "260000"],
            ["pbn_copy_kernel", "256", "300000", "310000"]]
    _write(str(tmp_path / "trace" / "run_kernel_trace.csv"), hdr, rows)
    out = str(tmp_path / "kt.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_trace_summary.py"), str(tmp_path / "trace"),
                    "--out", out], check=True, capture_output=True)
    d = json.load(open(out))
    assert d["dispatches"] == 2 and abs(d["avg_us"] - 22.0) < 1e-9


def test_handoff_summary_cuts_reps_at_gaps(tmp_path):
    """Two gated reps, the second followed (after a gap) by an untimed warm-up's dispatches: each
    rep is its gate's back-to-back dispatches; the rep with the extra copy is the hand-off's."""
    hdr = ["Kernel_Name", "Start_Timestamp", "End_Timestamp"]
    us = 1000
    rows = [["spin_kernel", 0, 100 * us],
            [PIPE, 101 * us, 181 * us], [PIPE, 181 * us, 261 * us],                     # bare rep
            ["spin_kernel", 300 * us, 400 * us],
            [PIPE, 401 * us, 491 * us], [PIPE, 491 * us, 581 * us], ["pbn_copy_kernel", 581 * us, 620 * us],
            [PIPE, 700 * us, 780 * us]]                                                 # next phase's warm-up
    _write(str(tmp_path / "h" / "run_kernel_trace.csv"), hdr, rows)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "handoff_trace.py"), "--summarize",
                        str(tmp_path / "h")], check=True, capture_output=True, text=True)
    d = json.loads(r.stdout)
    assert d["reps"] == 2
    assert len(d["median_rep"]["items"]) == 3 and abs(d["median_rep"]["span_us"] - 220.0) < 1e-6
    assert len(d["median_bare_rep"]["items"]) == 2 and abs(d["median_bare_rep"]["span_us"] - 161.0) < 1e-6


def _listing(order, cuid, body_b="v_add_u32_e32 v0, v1, v2"):
    """A device listing in the compiler's shape: two kernels in the given order (the function index
    in local labels follows the order), their descriptors, and the code object's metadata."""
    body = {"kern_a": "v_mov_b32_e32 v0, 0", "kern_b": body_b}
    out = ['\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"']
    for i, k in enumerate(order):
        out += ["\t.text", "\t.globl\t%s" % k, "\t.p2align\t8", "\t.type\t%s,@function" % k, "%s:" % k,
                "\t" + body[k], "\ts_cbranch_scc1 .LBB%d_2" % i, ".LBB%d_2:" % i, "\ts_endpgm",
                ".Lfunc_end%d:" % i, "\t.size\t%s, .Lfunc_end%d-%s" % (k, i, k), "\t.section\t.rodata",
                "\t.amdhsa_kernel %s" % k, "\t\t.amdhsa_next_free_vgpr 3", "\t.end_amdhsa_kernel", "\t.text",
                "; NumVgprs: 3"]
    out += ["\t.type\t__hip_cuid_%s,@object" % cuid, "__hip_cuid_%s:" % cuid, "\t.amdgpu_metadata", "---",
            "amdhsa.kernels:"]
    for k in order:
        out += ["  - .agpr_count:     0", "    .name:           %s" % k, "    .symbol:         %s.kd" % k,
                "    .vgpr_count:     3"]
    out += ["amdhsa.version:", "  - 1", "...", "\t.end_amdgpu_metadata"]
    return "\n".join(out) + "\n"


def test_listing_diff_compares_per_symbol():
    """tools/listing_diff.py: kernels that change their order in the file (and with it the function
    index of their labels) and the compilation unit's id compare equal; one changed instruction is
    reported for its kernel alone."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import listing_diff
    finally:
        sys.path.pop(0)
    a = _listing(["kern_a", "kern_b"], "1111")
    report, n = listing_diff.compare(a, _listing(["kern_b", "kern_a"], "2222"), 0)
    assert report == [] and n >= 4   # two kernels, their metadata entries, the file's head
    report, _ = listing_diff.compare(a, _listing(["kern_a", "kern_b"], "1111", "v_sub_u32_e32 v0, v1, v2"), 0)
    assert len(report) == 1 and "kern_b" in report[0] and "differs" in report[0]
    report, _ = listing_diff.compare(a, _listing(["kern_a"], "1111"), 0)
    assert any("only in THIS" in r and "kern_b" in r for r in report)
