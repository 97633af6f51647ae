"""Compare the gfx950 assembly of the library's kernels between two source trees, kernel by kernel.

  isa_diff.py asm <tree> <out_dir> [file.hip ...]    assembly of <tree>/cutrace_amd/csrc/<file.hip> -> <out_dir>/<file>.s, with
                                                     the flags of THIS tree's cutrace_amd/build.py (default: every .hip of the
                                                     tree's cutrace_amd/csrc that defines a kernel)
  isa_diff.py diff <parent_dir> <new_dir>            the table, then every differing line of every kernel that differs

A tree of another commit: `git archive <rev> | tar -x -C <dir>`.  Kernels are matched by their (mangled) name across all
the .s files of a directory, so a kernel that moved to another translation unit is still compared with itself.  Before the
comparison comments are stripped and local labels renumbered in order of appearance; the kernel's descriptor
(.amdhsa_kernel block: registers, LDS, scratch, kernarg size) is part of what is compared.  Text only: no instruction is
interpreted.
"""
import difflib
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_files(tree):
    """every .hip of the tree's cutrace_amd/csrc that defines a kernel"""
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(tree, "cutrace_amd", "csrc", "*.hip")) if "__global__" in open(p).read())


def make_asm(tree, out_dir, files):
    sys.path.insert(0, ROOT)
    from cutrace_amd import build
    flags = [f for f in build.HIP_FLAGS if not f.startswith("-I")]
    flags += ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, "cutrace_amd", "csrc")]
    os.makedirs(out_dir, exist_ok=True)
    jobs = []
    for f in files:
        src = os.path.join(tree, "cutrace_amd", "csrc", f)
        if not os.path.exists(src):
            print("(no %s in %s)" % (f, tree))
            continue
        out = os.path.join(out_dir, os.path.splitext(f)[0] + ".s")
        jobs.append((f, subprocess.Popen([build.hipcc(), *flags, "--offload-device-only", "-S", "-o", out, src])))
    for f, p in jobs:
        if p.wait() != 0:
            raise SystemExit("hipcc failed on " + f)


def kernels(directory):
    """name -> normalised lines of the kernel's code and descriptor, over every .s of the directory"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
        for name in names:
            a = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
            b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
            c = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\s*$", l))
            d = next(i for i in range(c, len(lines)) if ".end_amdhsa_kernel" in lines[i])
            out[name] = normalise(lines[a:b] + lines[c:d + 1])
    return out


def normalise(lines):
    body = []
    for l in lines:
        l = l.split(";")[0].rstrip()
        if l.strip():
            body.append(l)
    labels = {}

    def renumber(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    return [re.sub(r"\.L[A-Za-z_]+[0-9_]+", renumber, l) for l in body]


def short(name):
    m = re.search(r"render_kernelILj(\d+)E", name)
    if m:
        return "render_kernel<%s>" % m.group(1)
    try:
        return subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def diff(parent_dir, new_dir):
    P, N = kernels(parent_dir), kernels(new_dir)

    def order(name):
        m = re.search(r"render_kernelILj(\d+)E", name)
        return (0, int(m.group(1)), "") if m else (1, 0, short(name))
    print("%-58s %15s  %s" % ("kernel", "lines parent/new", "differing lines"))
    total, differing = 0, []
    for name in sorted(set(P) & set(N), key=order):
        d = [l for l in difflib.unified_diff(P[name], N[name], lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")]
        print("%-58s %7d/%-7d  %d" % (short(name)[:58], len(P[name]), len(N[name]), len(d)))
        total += 1
        if d:
            differing.append((name, d))
    print("\n%d kernels compared, %d with differing lines" % (total, len(differing)))
    print("only in parent:", sorted(short(n) for n in set(P) - set(N)) or "none")
    print("only in new:", sorted(short(n) for n in set(N) - set(P)) or "none")
    for name, d in differing:
        print("\n%s, every differing line:" % short(name))
        for l in d:
            print(l)
    return len(differing)


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "asm":
        make_asm(os.path.abspath(sys.argv[2]), sys.argv[3], sys.argv[4:] or kernel_files(os.path.abspath(sys.argv[2])))
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        diff(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
