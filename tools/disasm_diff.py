#!/usr/bin/env python3
"""Compare the device code of two builds of a library, function by function.

  python tools/disasm_diff.py OLD.so NEW.so [--show N]

Extracts the gfx950 code objects of both libraries (llvm-objdump --offloading), disassembles them (-d --no-show-raw-insn),
splits the text at every symbol, drops the address column and compares the instruction lists of equally named symbols.
Prints the number compared, the symbols only one side has and, for each symbol whose instructions differ, the opcodes whose
counts changed and a unified diff (at most N lines each, default 60).  Exit status 0: every symbol of OLD exists in NEW with
the same instructions.  A refactor that moves shared device code into a header should leave every kernel as it was; this is the check."""
import argparse
import collections
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ACX_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def functions_of(lib):
    """{symbol: [instruction text, ...]} over every amdgcn code object inside lib"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, stdout=subprocess.DEVNULL)
        for f in sorted(os.listdir(d)):
            if "amdgcn" not in f:
                continue
            dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f], cwd=d, text=True)
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    cur = out.setdefault(m.group(1), [])
                    continue
                if cur is None or not line.startswith(("\t", " ")):
                    continue
                text = line.split("//")[0].strip()          # the address (and a branch's resolved target) sit in the comment
                if text and text != "...":                  # (objdump's mark for a run of zero padding)
                    cur.append(text)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--show", type=int, default=60, help="diff lines printed per differing symbol")
    a = ap.parse_args()
    old, new = functions_of(a.old), functions_of(a.new)
    both = sorted(set(old) & set(new))
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differing = [s for s in both if old[s] != new[s]]
    print("symbols compared: %d (%d instructions), identical: %d, differing: %d, only in old: %d, only in new: %d"
          % (len(both), sum(len(old[s]) for s in both), len(both) - len(differing), len(differing), len(only_old), len(only_new)))
    for s in only_old:
        print("only in old: %s (%d instructions)" % (s, len(old[s])))
    for s in only_new:
        print("only in new: %s (%d instructions)" % (s, len(new[s])))
    for s in differing:
        d = list(difflib.unified_diff(old[s], new[s], "old", "new", lineterm="", n=2))
        print("differs: %s (%d -> %d instructions)" % (s, len(old[s]), len(new[s])))
        co, cn = (collections.Counter(x.split()[0] for x in side[s]) for side in (old, new))
        moved = ", ".join("%s %d -> %d" % (k, co[k], cn[k]) for k in sorted(set(co) | set(cn)) if co[k] != cn[k])
        print("    opcode counts: %s" % (moved or "equal (same instructions, other order or registers)"))
        for line in d[:a.show]:
            print("    " + line)
        if len(d) > a.show:
            print("    ... %d more diff lines" % (len(d) - a.show))
    return 1 if differing or only_old else 0


if __name__ == "__main__":
    sys.exit(main())
