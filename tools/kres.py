#!/usr/bin/env python3
"""Compact per-kernel resource table from hipcc's -Rpass-analysis=kernel-resource-usage remarks.
usage: tools/kres.py file.hip [extra hipcc flags]   (compiles for gfx950 into /tmp, prints name / VGPR / AGPR / SGPR / scratch / spills / LDS)"""
import re, subprocess, sys, os


def parse_remarks(stderr):
    """{mangled kernel name: {remark key: value}} in the order hipcc reported them (the one parser of these remarks: tools/codegen_diff.py uses it too)."""
    res, cur = {}, None
    for ln in stderr.splitlines():
        m = re.search(r"remark:\s+(.*?): (\S+)\s+\[-Rpass", ln) or re.search(r"remark:\s+(Function Name): (\S+)", ln)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = res.setdefault(v, {})
        elif cur is not None:
            cur[k] = v
    return res


def demangle(name):
    return subprocess.run(["c++filt", name], stdout=subprocess.PIPE, text=True).stdout.strip().replace("(anonymous namespace)::", "")


def main():
    src = sys.argv[1]
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", src, "-o", "/tmp/kres_%d.o" % os.getpid(),
           "-Rpass-analysis=kernel-resource-usage"] + sys.argv[2:]
    p = subprocess.run(cmd, stderr=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    for ln in p.stderr.splitlines():
        if "error" in ln and "remark:" not in ln: print(ln)
    print("%-5s %-5s %-5s %-8s %-7s %-7s %-6s %s" % ("VGPR", "AGPR", "SGPR", "scratch", "vspill", "sspill", "occ", "kernel"))
    for name, r in parse_remarks(p.stderr).items():
        print("%-5s %-5s %-5s %-8s %-7s %-7s %-6s %s" % (r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"), r.get("VGPRs Spill"), r.get("SGPRs Spill"),
                                                       r.get("Occupancy [waves/SIMD]"), demangle(name)[:110]))
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
