"""Compare the instruction streams of kernels between two device-only assembly listings of one
translation unit (hipcc --cuda-device-only -S), function by function.

    python tools/isa_compare.py before.s after.s [--grep k_mlp] [--drop GridOne]

A function's stream is its instruction lines with comments, assembler directives and the numbers of
basic-block labels stripped (a label's number moves when another function is added to the unit).
Functions are paired by demangled name after every --drop argument has been removed from the name's
template arguments (a template that gained a defaulted parameter keeps its pairing).  Prints one line
per pair -- instruction counts and "identical" or the first differing line -- and the functions only
one side has; exits 1 if any pair differs.  No GPU needed.
"""
import argparse
import re
import subprocess
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if re.match(r"^\s*\.end_amdhsa_kernel|^\.Lfunc_end", line):
            name = None
            continue
        text = line.split(";")[0].strip()
        if not text or text.startswith("."):
            if re.match(r"^\.LBB\d+_\d+:", text):
                body.append("LABEL:")
            continue
        body.append(re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", text))
    return {k: v for k, v in out.items() if v}


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(names)


def keyed(path, grep, drops):
    fs = functions(path)
    names = list(fs)
    out = {}
    for n, d in zip(names, demangle(names)):
        if grep not in d:
            continue
        d = re.sub(r">\((?!anonymous).*$", ">", d)            # the parameter list
        for x in drops:
            d = re.sub(r",\s*(\(anonymous namespace\)::)?" + re.escape(x) + r"\s*>", ">", d)
        out[d.replace(" ", "")] = fs[n]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--grep", default="")
    ap.add_argument("--drop", action="append", default=[])
    a = ap.parse_args()
    A, B = keyed(a.before, a.grep, a.drop), keyed(a.after, a.grep, a.drop)
    bad = 0
    for k in sorted(set(A) & set(B)):
        if A[k] == B[k]:
            print(f"identical  {len(A[k]):6d} instructions  {k}")
        else:
            bad += 1
            i = next((i for i, (x, y) in enumerate(zip(A[k], B[k])) if x != y), min(len(A[k]), len(B[k])))
            print(f"DIFFERENT  {len(A[k]):6d} -> {len(B[k]):6d}  {k}\n    first difference at line {i}: "
                  f"{A[k][i] if i < len(A[k]) else '<end>'!r} -> {B[k][i] if i < len(B[k]) else '<end>'!r}")
    for k in sorted(set(A) - set(B)):
        print(f"only before  {k}")
    for k in sorted(set(B) - set(A)):
        print(f"only after   {len(B[k]):6d} instructions  {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
