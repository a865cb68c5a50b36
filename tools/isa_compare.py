#!/usr/bin/env python3
"""Device code of two source trees compared kernel by kernel, without a GPU (the check behind a pure code move).

  tools/isa_compare.py asm CSRC_DIR OUT_DIR     device assembly of every .hip unit in CSRC_DIR into OUT_DIR/*.s, with the flags of CSRC_DIR's own
                                                Makefile (`make -pn`, so ARCH and EXTRA given in the environment count)
  tools/isa_compare.py diff OLD_DIR NEW_DIR     one line per kernel symbol over all units together: identical, allowed or changed

Per kernel the instruction text, the .amdhsa_* directives and the scalar entries of the code object metadata are compared, after
dropping comments, .file / .loc / .ident lines, the unit's __hip_cuid_* symbol and the per-unit numbering of local labels.
`allowed`: the text differs, but the instruction count, the multiset of opcodes and every resource number are the same (a constant or
a register moved).  Everything else that differs is `changed`; a kernel in one tree only is `missing` / `added`.  Exit status 1 unless
every kernel is identical or allowed."""
import collections
import glob
import os
import re
import subprocess
import sys

SHOWN = ((".vgpr_count", "vgpr"), (".agpr_count", "agpr"), (".sgpr_count", "sgpr"), (".private_segment_fixed_size", "scratch"), (".group_segment_fixed_size", "lds"))


def asm(csrc, out):
    os.makedirs(out, exist_ok=True)
    db = subprocess.run(["make", "-C", csrc, "-pn"], capture_output=True, text=True).stdout
    var = lambda name: re.search(r"^%s :?= (.*)$" % name, db, re.M).group(1)
    flags = var("HIPFLAGS").replace("$(ARCH)", var("ARCH")).replace("$(CXXFLAGS)", var("CXXFLAGS")).replace("$(EXTRA)", os.environ.get("EXTRA", ""))
    flags = flags.replace("-I../../include", "-I" + os.path.join(csrc, "..", "..", "include"))
    jobs = [subprocess.Popen([var("HIPCC"), *flags.split(), "--cuda-device-only", "-S", u, "-o", os.path.join(out, os.path.basename(u) + ".s")])
            for u in sorted(glob.glob(os.path.join(csrc, "*.hip")))]
    return max(p.wait() for p in jobs)


def kernels(directory):
    """{symbol: (unit, instruction lines, {directive or metadata key: value})} over every .s of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        text, start = {}, {}
        name = None
        for i, raw in enumerate(lines):
            m = re.match(r"^(\w+):", raw)
            if m and i and lines[i - 1].strip().startswith(".type") and "@function" in lines[i - 1]:
                name, text[m.group(1)] = m.group(1), []
                continue
            if name is None:
                continue
            s = raw.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                name = None
            elif s and not re.match(r"\.(file|loc|ident|section|p2align|text)\b", s) and "__hip_cuid_" not in s:
                text[name].append(re.sub(r"\.L(BB|tmp|func_end)\d+", r".L\1", s))
        for i, raw in enumerate(lines):
            m = re.match(r"\s*\.amdhsa_kernel (\S+)", raw)
            if m:
                start[m.group(1)] = i
        meta, cur = {}, None
        in_meta = False
        for raw in lines:
            if raw.strip() == ".amdgpu_metadata":
                in_meta = True
            elif raw.startswith("  - ."):
                cur = {}
                raw = "    " + raw[4:]
            if in_meta and cur is not None:
                m = re.match(r"^    (\.\w+):\s+(\S.*)$", raw)
                if m:
                    cur[m.group(1)] = m.group(2)
                    if m.group(1) == ".name":
                        meta[m.group(2)] = cur
        for sym, i in start.items():
            res = {k: v for k, v in meta[sym].items() if k != ".symbol"}
            j = i + 1
            while ".end_amdhsa_kernel" not in lines[j]:
                k, v = lines[j].split()
                res[k] = v
                j += 1
            body = [l for l in text[sym] if not l.startswith(".amdhsa_") and not l.startswith(".end_amdhsa") and not l.startswith(".amdhsa_kernel")]
            out[sym] = (os.path.basename(path)[:-2], body, res)
    return out


def diff(old_dir, new_dir):
    old, new = kernels(old_dir), kernels(new_dir)
    tally = collections.Counter()
    syms = sorted(set(old) | set(new))
    try:  # readable names where the demangler is installed
        names = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        names = {}
    for sym in syms:
        if sym not in old or sym not in new:
            verdict = "missing" if sym not in new else "added"
            unit, body, res = old.get(sym) or new.get(sym)
            where = unit
        else:
            (u0, b0, r0), (unit, body, res) = old[sym], new[sym]
            ops = lambda b: collections.Counter(l.split()[0] for l in b if not l.endswith(":"))
            where = unit if u0 == unit else u0 + " -> " + unit
            if b0 == body and r0 == res:
                verdict = "identical"
            elif r0 == res and len(b0) == len(body) and ops(b0) == ops(body):
                verdict = "allowed  "
            else:
                verdict = "changed  "
                where += "  (was: %d lines, %s)" % (len(b0), " ".join("%s %s" % (n, r0[k]) for k, n in SHOWN))
        tally[verdict.strip()] += 1
        print("%s %5d lines  %s  %s  [%s]" % (verdict, len(body), " ".join("%s %3s" % (n, res[k]) for k, n in SHOWN), names.get(sym, sym), where))
    print("total:", ", ".join("%d %s" % (n, v) for v, n in sorted(tally.items())))
    return 0 if set(tally) <= {"identical", "allowed"} else 1


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] not in ("asm", "diff"):
        sys.exit(__doc__)
    sys.exit(asm(sys.argv[2], sys.argv[3]) if sys.argv[1] == "asm" else diff(sys.argv[2], sys.argv[3]))
