"""What the gpu_*.py measurement scripts share: the compiler's resource report of a kernel's instantiations, and the
HIP-event timing of a call."""
import os
import re
import statistics
import subprocess

REMARK = re.compile(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize|Occupancy|LDS Size|TotalSGPRs)(?: \[[^\]]*\])?: (\S+)")


def resource_report(source, kernel, flag_names, plain, footnote, csrc=None, by_number=False):
    """The text of a --resources report: per instantiation of the template `kernel` in <csrc>/<source> (default: this tree's
    cutrace_amd/csrc), "kernel<bits> (NAMES)" and the compiler's figures, then `footnote`.  flag_names: ((bit, name), ...)
    for NAMES, `plain` when no bit is set.  Blocks come in the compiler's order, another function as kernel<-1>; by_number:
    sorted by bits instead (a new instantiation adds a block and moves no other), other functions left out."""
    from cutrace_amd import build as b
    csrc = csrc or b.CSRC
    flags = [f for f in b.HIP_FLAGS if f != "-I" + b.CSRC] + ["-I" + csrc]
    cmd = [b.hipcc(), *flags, "--offload-device-only", "-c", "-o", os.devnull, os.path.join(csrc, source),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, check=True)
    blocks, cur = [], None
    for line in r.stderr.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        key, val = m.group(1), m.group(2)
        if key == "Function Name":
            v = re.search(kernel + r"ILj(\d+)E", val)
            cur = None
            if v or not by_number:
                cur = (int(v.group(1)) if v else -1, [])
                blocks.append(cur)
        elif cur is not None:
            cur[1].append(f"    {key}: {val}")
    if by_number:
        blocks.sort(key=lambda block: block[0])
    lines = []
    for bits, figures in blocks:
        lines.append(f"{kernel}<{bits}> ({' | '.join(n for bit, n in flag_names if bits & bit) or plain})")
        lines += figures
    return "\n".join(lines) + footnote


def write_report(out, name, txt):
    with open(os.path.join(out, name), "w") as f:
        f.write(txt)
    print(txt)


def timed(fn, reps, warmup):
    """(median, min, max) HIP-event milliseconds of fn() over `reps` calls after `warmup` calls."""
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts), min(ts), max(ts)
