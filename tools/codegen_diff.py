#!/usr/bin/env python3
"""Per-kernel generated-code comparison of two source trees: the evidence a refactor that must not change the kernels commits.
usage: tools/codegen_diff.py OLD_CSRC NEW_CSRC file.hip [file.hip ...] [--allow-removed]   (e.g. OLD_CSRC = `git worktree add` of the parent, NEW_CSRC = mlx_audio_amd/csrc)
--allow-removed: kernels that exist only in OLD_CSRC are listed, not counted as a failure (a change that deletes kernels); new ones still fail.

Every file is compiled for gfx950 to assembly with exactly build.py's flags (COMMON_FLAGS and the file's EXTRA_FLAGS).  Per kernel it compares
  * the resources of hipcc's kernel-resource-usage remarks (VGPRs, AGPRs, SGPRs, scratch, spills, LDS, occupancy): must be equal;
  * the count of every mnemonic of the FIXED groups (matrix, fp32 multiply / add / fma, transcendental, convert, global and LDS memory): must be
    equal -- a difference there means a floating-point operation or a memory access was added, dropped, reordered or re-fused;
  * every other mnemonic (integer, address, move, wait, branch): differences are listed, they do not fail the comparison.
A kernel whose instructions are the same text in the same order, registers and labels included, is marked so.
Exit status 1 if any kernel fails."""
import collections, os, re, subprocess, sys, tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mlx_audio_amd.build import COMMON_FLAGS, EXTRA_FLAGS, _hipcc
from tools.kres import demangle, parse_remarks

FIXED = re.compile(r"^(v_mfma|v_fma|v_fmac|v_mul_f32|v_add_f32|v_sub_f32|v_exp|v_rcp|v_div|v_cvt|global_load|global_store|ds_)")
RES = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]


def compile_one(csrc, name, out):
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", *COMMON_FLAGS, *EXTRA_FLAGS.get(name, []), "-x", "hip", "--cuda-device-only", "-S",
           os.path.join(csrc, name), "-o", out, "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        sys.exit(p.stderr)
    res = parse_remarks(p.stderr)
    hist, body, cur = {}, {}, None
    for ln in open(out):
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in res:
            cur = m.group(1)
            hist[cur], body[cur] = collections.Counter(), []
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            m = re.match(r"^\s+([a-z][a-z0-9_]+)(\s|$)", ln)
            if m:
                hist[cur][m.group(1)] += 1
                body[cur].append(ln.split(";")[0].strip())
    return res, hist, body


def main():
    argv = [x for x in sys.argv[1:] if x != "--allow-removed"]
    allow_removed = len(argv) != len(sys.argv) - 1
    old, new, files = argv[0], argv[1], argv[2:]
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name in files:
            r0, h0, t0 = compile_one(old, name, os.path.join(tmp, "old.s"))
            r1, h1, t1 = compile_one(new, name, os.path.join(tmp, "new.s"))
            print("== %s: %d kernels" % (name, len(r1)))
            if set(r0) != set(r1):
                removed_only = allow_removed and not set(r1) - set(r0)
                bad += not removed_only
                print("   %s kernel symbols differ: only old %s, only new %s" % ("removed" if removed_only else "FAIL",
                      sorted(demangle(k) for k in set(r0) - set(r1)), sorted(demangle(k) for k in set(r1) - set(r0))))
            for k in sorted(set(r0) & set(r1)):
                dem = demangle(k)
                resd = [(q, r0[k].get(q), r1[k].get(q)) for q in RES if r0[k].get(q) != r1[k].get(q)]
                diff = [(mn, h0[k][mn], h1[k][mn]) for mn in sorted(set(h0[k]) | set(h1[k])) if h0[k][mn] != h1[k][mn]]
                fixed = [d for d in diff if FIXED.match(d[0])]
                ok = not resd and not fixed
                bad += not ok
                print("   %-4s %s%s" % ("ok" if ok else "FAIL", dem[:150], "   [instruction stream identical]" if t0[k] == t1[k] else ""))
                print("        " + "  ".join("%s=%s" % (q.split(" [")[0].replace(" ", "_"), r1[k].get(q)) for q in RES) + "  instructions=%d (old %d)" % (sum(h1[k].values()), sum(h0[k].values())))
                for q, a, b in resd:
                    print("        RESOURCE %s: %s -> %s" % (q, a, b))
                for mn, a, b in diff:
                    print("        %s %s: %d -> %d" % ("FIXED-GROUP" if FIXED.match(mn) else "other", mn, a, b))
    print("== %s" % ("all kernels equal in resources and fixed-group instruction counts" if not bad else "%d FAILURES" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
