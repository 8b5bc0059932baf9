#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel.

    hipcc <the Makefile's flags for the file> --cuda-device-only -S file.hip -o DIR/file.s      (once per build)
    python tools/asm_compare.py DIR_A DIR_B

Every *.s of the two directories (sub-directories included; one present on one side only is reported) is split per function symbol; comment lines,
trailing comments and directives that carry no instruction are dropped, labels and instructions are kept (block labels without the
function's index in its file, which shifts when a kernel is added in front of it).  Prints
one line per kernel -- identical / differs (with the instruction counts) / only in one build -- and a total.
Exit status 1 if anything differs.
"""
import os
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if name is None:
            m = re.match(r"^([A-Za-z_$][\w$.]*):$", s)
            if m and not s.startswith(".L"):
                name, body = m.group(1), []
            continue
        if s.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        if s.startswith(".") and not s.endswith(":"):
            continue  # directive
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))  # (block labels carry the function's index in its file: a kernel added in front shifts it)
    if name is not None:
        print(f"warning: {path}: function {name} has no .Lfunc_end label, skipped", file=sys.stderr)
    return out


def s_files(d):
    return {os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs if f.endswith(".s")}


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    in_a, in_b = s_files(a_dir), s_files(b_dir)
    same = diff = 0
    for f in sorted(in_a | in_b):
        if f not in in_a or f not in in_b:
            print(f"{f}: only in {a_dir if f in in_a else b_dir}")
            diff += 1
            continue
        fa, fb = functions(os.path.join(a_dir, f)), functions(os.path.join(b_dir, f))
        for k in sorted(set(fa) | set(fb)):
            if k not in fa or k not in fb:
                print(f"{f}  {k}: only in {a_dir if k in fa else b_dir}")
                diff += 1
            elif fa[k] == fb[k]:
                print(f"{f}  {k}: identical ({len(fa[k])} lines)")
                same += 1
            else:
                print(f"{f}  {k}: DIFFERS ({len(fa[k])} vs {len(fb[k])} lines)")
                diff += 1
    print(f"total: {same} identical, {diff} differ")
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
