"""Per-kernel table of vector loads and the full waits behind them, from the device assembly of a HIP translation unit (compiled
with the Makefile's flags; a `.s` file is read as it is).  Four numbers per kernel:
  instr   instructions
  loads   vector memory loads (global_load_* / flat_load_* / buffer_load_*)
  tight   loads followed within two instructions by a full wait, `s_waitcnt vmcnt(0)`: a load that travels alone
  inloop  full waits between a label and a backward branch to it: paid once per trip
A full wait after a GROUP of loads is one round trip for the group; `tight` counts the loads that are their own group.  The tool
counts loads and waits, nothing else.
usage: python tools/load_waits.py chainpartitioners.jl_amd/csrc/dp_total_own.hip [name-substring ...]   (one unit per call, the one that
       names the kernel: dp_total_own.hip for k_lpass_own / k_fix_own / k_own_map, dp_total.hip for k_setup_short and the flattened
       stage's k_lpass, dp_total_rounda.hip for k_ra_* / k_win_*, dp_total_rpass.hip for k_rpass_*, dp_total_gap.hip for k_gap_*,
       dp_total_leaf.hip for k_leaf)"""
import re
import subprocess
import sys

from kernel_text import makefile_flags
from resource_usage import demangle

LOAD = re.compile(r"(global|flat|buffer)_load_")
FULL = re.compile(r"s_waitcnt\b.*\bvmcnt\(0\)")
BRANCH = re.compile(r"s_c?branch\w*\s+(\.LBB\w+)")


def kernels(asm):
    """name -> list of body lines (labels and instructions), for every kernel of the assembly text."""
    is_kernel = set(re.findall(r"\.amdhsa_kernel\s+(\S+)", asm))
    out, name, body = {}, None, []
    for line in asm.split("\n"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.split(";")[0].strip()
        if re.match(r"\.Lfunc_end\d+:", t):
            if name in is_kernel:
                out[name] = body
            name = None
        elif t and (not t.startswith(".") or re.match(r"\.LBB\w+:", t)) and t != name + ":":
            body.append(t)
    return out


def count(body):
    ins = [t for t in body if not t.endswith(":")]
    loads = [i for i, t in enumerate(ins) if LOAD.match(t)]
    tight = sum(1 for i in loads if any(FULL.match(t) for t in ins[i + 1:i + 3]))
    # loops: a branch to a label that lies above it
    at, inloop = {}, set()
    for i, t in enumerate(body):
        if t.endswith(":"):
            at[t[:-1]] = i
    for i, t in enumerate(body):
        m = BRANCH.match(t)
        if m and at.get(m.group(1), i) < i:
            inloop.update(j for j in range(at[m.group(1)], i) if FULL.match(body[j]))
    return len(ins), len(loads), tight, len(inloop)


def main():
    src, pats = sys.argv[1], sys.argv[2:]
    if src.endswith(".s"):
        asm = open(src).read()
    else:
        asm = subprocess.run(makefile_flags() + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True).stdout
    ks = kernels(asm)
    syms = sorted(ks)
    names = [re.sub(r"^void ", "", re.sub(r"\(.*", "", n)) for n in demangle(syms)]
    print(f"{'kernel':70s} {'instr':>6s} {'loads':>6s} {'tight':>6s} {'inloop':>7s}")
    for sym, nm in sorted(zip(syms, names), key=lambda x: x[1]):
        if pats and not any(p in nm for p in pats):
            continue
        print(f"{nm[:70]:70s} " + "{:6d} {:6d} {:6d} {:7d}".format(*count(ks[sym])))


if __name__ == "__main__":
    main()
