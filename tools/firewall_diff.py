"""Compares the device functions of two builds of one .hip file, instruction text only: the check
that a change meant for new kernel instantiations left the existing ones alone (every kernel edit
moves the register allocator of whatever it touches by 1-10 %).

  hipcc <the Makefile's flags> --save-temps -c csrc/trace_kernel.hip     (once per tree)
  python tools/firewall_diff.py PARENT.s BRANCH.s [--drop-arg N]

PARENT.s / BRANCH.s are the device assembly files --save-temps leaves (…-hip-amdgcn-amd-amdhsa-gfx950.s).
Per function (the text between its label and its .Lfunc_end), comments, directives and blank lines
are dropped and the function-indexed labels (.LBB<n>_, .Lfunc_end<n>) normalised. A trailing
defaulted template argument added by the branch shows in the mangled names of its instantiations of
existing kernels as one more ELb0: --drop-arg strips that from the branch's names (default on).
Prints the functions only in one file, the functions that differ, and exits 1 if any parent
function is missing or differs.
"""
import argparse
import re
import sys


def functions(path, strip_trailing_false):
    out, name, body = {}, None, []
    label = re.compile(r"^([A-Za-z_][\w.$]*):")
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = label.match(line)
        if m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if line.strip().startswith(".Lfunc_end"):
            key = name
            if strip_trailing_false:
                key = re.sub(r"ELb0EEEvNS_9TraceArgsE$", "EEEvNS_9TraceArgsE", key)
            out[key] = body
            name = None
            continue
        if line.strip().startswith(".") and not line.strip().startswith(".LBB"):
            continue   # directives
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        if strip_trailing_false:
            line = re.sub(r"ELb0EEEvNS_9TraceArgsE", "EEEvNS_9TraceArgsE", line)
        body.append(line.strip())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--keep-arg", action="store_true", help="do not strip the branch's trailing ELb0")
    args = ap.parse_args()
    a = functions(args.parent, False)
    b = functions(args.branch, not args.keep_arg)
    missing = sorted(set(a) - set(b))
    new = sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print(f"parent {len(a)} functions, branch {len(b)}; {len(a) - len(missing) - len(differ)} identical, "
          f"{len(differ)} differ, {len(missing)} missing, {len(new)} new")
    for k in differ:
        n = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        print(f"  differs: {k} ({len(a[k])} vs {len(b[k])} instructions, first at {n})")
    for k in missing:
        print(f"  missing: {k}")
    for k in new:
        print(f"  new: {k} ({len(b[k])} instructions)")
    sys.exit(1 if differ or missing else 0)


if __name__ == "__main__":
    main()
