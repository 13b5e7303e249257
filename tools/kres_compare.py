#!/usr/bin/env python
"""Compare the code objects of two builds of the same .hip files, kernel by kernel (no GPU needed).
    python tools/kres_compare.py DIR_BEFORE DIR_AFTER > table.txt
Each directory holds, per file NAME.hip, NAME.s and NAME.remarks as written by
    hipcc -O3 -std=c++17 --offload-arch=gfx950 [the file's Makefile flags] --cuda-device-only -S NAME.hip -o DIR/NAME.s \\
          -Rpass-analysis=kernel-resource-usage 2> DIR/NAME.remarks
Per kernel: VGPRs, SGPRs, scratch, LDS and the occupancy limit from the remarks; from the assembly the number of v_mfma,
buffer_load_dwordx4 and global_store_dwordx4 instructions, the multiset of s_waitcnt vmcnt(N) literals inside inline asm
("hand-counted") and outside it ("compiler"), and the instruction count.  A line is marked DIFF when a quantity that must be equal
is not (VGPRs, scratch, LDS, occupancy, the three instruction counts, the hand-counted waits) and "waits" / "sgpr" when only the
compiler's waits or the SGPRs moved; the last lines summarise."""
import collections
import glob
import os
import re
import subprocess
import sys


def remarks(path):
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = rows.setdefault(t.split(": ", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return rows


def assembly(path):
    out, name, in_asm = {}, None, False
    for line in open(path):
        s = line.strip()
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            name = m.group(1)
            out[name] = {"mfma": 0, "bl": 0, "gs": 0, "hand": collections.Counter(), "comp": collections.Counter(), "n": 0}
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            name = None
            continue
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not s or s[0] in ".;" or s.endswith(":"):
            continue
        k = out[name]
        k["n"] += 1
        op = s.split()[0]
        if op.startswith("v_mfma"):
            k["mfma"] += 1
        elif op == "buffer_load_dwordx4":
            k["bl"] += 1
        elif op == "global_store_dwordx4":
            k["gs"] += 1
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                k["hand" if in_asm else "comp"][int(m.group(1))] += 1
    return out


def ms(c):
    return "{" + ",".join("%d:%d" % kv for kv in sorted(c.items())) + "}"


def main(a_dir, b_dir):
    n = bad = waits = sgpr = same_n = 0
    for sa in sorted(glob.glob(os.path.join(a_dir, "*.s"))):
        base = os.path.basename(sa)[:-2]
        ra, rb = remarks(os.path.join(a_dir, base + ".remarks")), remarks(os.path.join(b_dir, base + ".remarks"))
        aa, ab = assembly(sa), assembly(os.path.join(b_dir, base + ".s"))
        assert sorted(ra) == sorted(rb), (base, "the two builds instantiate different kernels", sorted(set(ra) ^ set(rb)))
        names = subprocess.run(["c++filt"], input="\n".join(ra), capture_output=True, text=True).stdout.split("\n")
        for mangled, nice in sorted(zip(ra, names), key=lambda t: t[1]):
            x, y, p, q = ra[mangled], rb[mangled], aa[mangled], ab[mangled]
            nice = re.sub(r"^void rtod::|_kernel|\(.*$", "", nice)
            g = lambda d, k: d.get(k, "?")
            must = [(g(x, k), g(y, k)) for k in ("VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")]
            must += [(p[k], q[k]) for k in ("mfma", "bl", "gs", "hand")]
            flag = "DIFF" if any(u != v for u, v in must) or g(y, "ScratchSize [bytes/lane]") != "0" else ""
            if not flag and p["comp"] != q["comp"]:
                flag = "waits"
            if not flag and g(x, "TotalSGPRs") != g(y, "TotalSGPRs"):
                flag = "sgpr"
            n += 1
            bad += flag == "DIFF"
            waits += p["comp"] != q["comp"]
            sgpr += g(x, "TotalSGPRs") != g(y, "TotalSGPRs")
            same_n += p["n"] == q["n"]
            print("%-62s vgpr %3s -> %3s, sgpr %3s -> %3s, scratch %s -> %s, lds %6s -> %6s, occupancy %s -> %s | mfma %3d -> %3d, buffer_load_dwordx4 %2d -> %2d, "
                  "global_store_dwordx4 %2d -> %2d, hand-counted vmcnt %s -> %s, compiler vmcnt %s -> %s, instructions %5d -> %5d  %s"
                  % (nice[:62], g(x, "VGPRs"), g(y, "VGPRs"), g(x, "TotalSGPRs"), g(y, "TotalSGPRs"), g(x, "ScratchSize [bytes/lane]"), g(y, "ScratchSize [bytes/lane]"),
                     g(x, "LDS Size [bytes/block]"), g(y, "LDS Size [bytes/block]"), g(x, "Occupancy [waves/SIMD]"), g(y, "Occupancy [waves/SIMD]"),
                     p["mfma"], q["mfma"], p["bl"], q["bl"], p["gs"], q["gs"], ms(p["hand"]), ms(q["hand"]), ms(p["comp"]), ms(q["comp"]), p["n"], q["n"], flag))
    print("# %d kernels; %d DIFF (VGPRs, scratch, LDS, occupancy, v_mfma / buffer_load_dwordx4 / global_store_dwordx4 counts or hand-counted waits); "
          "compiler waits differ in %d, SGPRs in %d; instruction counts equal in %d" % (n, bad, waits, sgpr, same_n))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
