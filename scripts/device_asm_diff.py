#!/usr/bin/env python
"""Compare the device code of two builds of one HIP source, kernel by kernel.

    hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S csrc/dgp_conv_split.hip -o new.s      (same at the parent: old.s)
    python scripts/device_asm_diff.py old.s new.s
    python scripts/device_asm_diff.py old.s -- a.s b.s c.s      (a source split into several: each side is the union of its files)
    python scripts/device_asm_diff.py --drop-arg conv_igemm_split_ls:6 old.s new.s      (new.s removed the function's 6th template parameter)

Splits each assembly file into its functions, keeps the instruction text (no directives, no comments) and drops the function-index part
of local labels (.LBB<fn>_<n>, which moves when host-only edits reorder the instantiations).  Prints the functions only one side has
and the ones whose instructions differ; exit status 1 if there are any.  Metadata (amdhsa.kernels: the order of the entries) is not
compared.  A function that more than one file of a side defines is reported as well.  --drop-arg NAME:N removes the N-th (1-based, literal)
template argument of function NAME from the FIRST side's mangled names before matching."""
import re
import sys

LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end)\d+(_\d+)?")


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w.$]*):\s*(;.*)?$", line)
        if m and not m.group(1).startswith(".L"):
            if name:
                out[name] = body
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        t = line.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            out[name], name = body, None
        elif t and not t.startswith("."):
            body.append(LABEL.sub(lambda q: ".L" + q.group(1) + (q.group(2) or ""), t))
    if name:
        out[name] = body
    return {k: v for k, v in out.items() if v and not k.startswith(("__hip_cuid", "amdhsa."))}


def side(paths):
    out, twice = {}, []
    for p in paths:
        f = functions(p)
        twice += sorted(set(f) & set(out))
        out.update(f)
    return out, twice


def main(a_paths, b_paths, drop=None):
    (a, a2), (b, b2) = side(a_paths), side(b_paths)
    if drop:
        name, n = drop.rsplit(":", 1)
        arg = re.compile(r"(%d%sI(?:L[^E]*E){%d})L[^E]*E" % (len(name), name, int(n) - 1))
        a = {arg.sub(r"\1", k): v for k, v in a.items()}
    a_path, b_path = " ".join(a_paths), " ".join(b_paths)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    print("%d / %d functions, %d / %d instructions" % (len(a), len(b), sum(map(len, a.values())), sum(map(len, b.values()))))
    for what, names in (("only in " + a_path, only_a), ("only in " + b_path, only_b), ("instructions differ", differ),
                        ("defined in more than one file of a side", a2 + b2)):
        print("%s: %d" % (what, len(names)))
        for n in names:
            print("   ", n)
    return 1 if only_a or only_b or differ or a2 or b2 else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    drop = args.pop(args.index("--drop-arg") + 1) if "--drop-arg" in args else None
    args = [x for x in args if x != "--drop-arg"]
    cut = args.index("--") if "--" in args else 1
    sys.exit(main(args[:cut], [x for x in args[cut:] if x != "--"], drop))
