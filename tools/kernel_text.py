"""One line `symbol sha1` per device function of one or more HIP translation units, sorted: the check that a host-only change left
the device code alone (same symbols, same hashes before and after).  Each unit is compiled with the Makefile's flags to device
assembly; a function's text runs from `.type SYM,@function` to its `.Lfunc_end`, with the ordinals of local labels removed (they
count functions and blocks in instantiation order, which host edits move), comment / debug-location lines dropped and trailing
comments cut (the assembler pads them to a column that depends on the digits of the label in front: `.LBB24_9:   ; =>This Inner
Loop Header` moves when the function's ordinal goes from one digit to two).  Text is hashed, no instruction is inspected.  Several
units give one table; a symbol defined by two of them is an error.
usage: python tools/kernel_text.py chainpartitioners.jl_amd/csrc/dp_total.hip [chainpartitioners.jl_amd/csrc/dp_total_gap.hip ...]
       (the total-cost DP as one table: chainpartitioners.jl_amd/csrc/dp_total*.hip)"""
import hashlib
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "chainpartitioners.jl_amd", "csrc")


def makefile_flags():
    """HIPCC and FLAGS as the Makefile spells them ($(ARCH) expanded)."""
    var = {}
    for line in open(os.path.join(CSRC, "Makefile")):
        m = re.match(r"(\w+)\s*\??=\s*(.*)", line)
        if m:
            var[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda r: var.get(r.group(1), ""), m.group(2).strip())
    return [var["HIPCC"]] + var["FLAGS"].split()


def cut_comment(line):
    """The line without its trailing `; comment` and the blanks in front of it; a `;` inside a quoted string (data directives) stays."""
    quoted, i = False, 0
    while i < len(line):
        c = line[i]
        if quoted and c == "\\":
            i += 1
        elif c == '"':
            quoted = not quoted
        elif c == ";" and not quoted:
            return line[:i].rstrip()
        i += 1
    return line


def kernel_hashes(src):
    asm = subprocess.run(makefile_flags() + ["--cuda-device-only", "-S", src, "-o", "-"], capture_output=True, text=True, check=True).stdout
    out, name, body = {}, None, []
    for line in asm.split("\n"):
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.strip()
        if t.startswith(";") or re.match(r"\.(loc|file|cfi_\w+)\b", t):
            continue
        body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end)[0-9_]+", r".L\1", cut_comment(line)))
        if re.match(r"\.Lfunc_end\d+:", t):
            out[name] = hashlib.sha1("\n".join(body).encode()).hexdigest()
            name = None
    return out


def unit_hashes(srcs):
    """The table of several units together: {symbol: hash}; a symbol two units define is an error."""
    out, owner = {}, {}
    for src in srcs:
        for sym, h in kernel_hashes(src).items():
            if sym in out:
                sys.exit("%s is defined by %s and by %s" % (sym, owner[sym], src))
            out[sym], owner[sym] = h, src
    return out


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    for sym, h in sorted(unit_hashes(sys.argv[1:]).items()):
        print(sym, h)
