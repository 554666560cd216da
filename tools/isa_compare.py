"""Compare the gfx950 ISA of two builds of one translation unit, kernel by kernel.

usage: isa_compare.py parent.s new.s      (both from: hipcc <the build's flags, without -fPIC> --cuda-device-only -S)

Per kernel it prints one of
  IDENTICAL   the kernel's text is the same line for line
  PIPELINE    the text differs, but between the kernel's first and last s_barrier the instruction count is the same
              and the pipeline instructions (MFMA, LDS reads, LDS-DMA, s_waitcnt, s_barrier, s_setprio, s_sleep,
              branches) are the same sequence once register numbers are masked
  LOOPS       neither, but every basic block that holds an MFMA -- the bodies and tails of the ring loops -- is the same
              instruction sequence once register numbers and labels are masked: what changed lies in the prologue and
              the epilogue (epilogue code that the scheduler places ahead of the loop's closing barrier counts into
              the PIPELINE region and fails that test)
  DIFFERENT   anything else
and exits 1 when a kernel is DIFFERENT or missing."""
import re
import sys

PIPE = ("v_mfma", "ds_read", "ds_load", "global_load_lds", "buffer_load", "s_waitcnt", "s_barrier", "s_setprio", "s_sleep",
        "s_cbranch", "s_branch")


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if line.startswith(".Lfunc_end"):
            name = None
        if name is not None and "__hip_cuid" not in line:
            out[name].append(line.rstrip())
    return out


def region(lines):
    ins = [l.split(";")[0].strip() for l in lines]
    ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
    idx = [i for i, l in enumerate(ins) if l.startswith("s_barrier")]
    if len(idx) < 2:
        return len(ins), [l for l in ins if l.startswith(PIPE)]
    reg = ins[idx[0]:idx[-1] + 1]
    mask = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", l) for l in reg]
    return len(reg), [l for l in mask if l.startswith(PIPE)]


def mfma_blocks(lines):
    out, cur = [], []
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            if t.endswith(":") and cur:
                out.append(cur)
                cur = []
            continue
        cur.append(re.sub(r"\.LBB\d+_\d+", ".L", re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", t)))
        if t.startswith(("s_cbranch", "s_branch")):
            out.append(cur)
            cur = []
    out.append(cur)
    return [b for b in out if any(i.startswith("v_mfma") for i in b)]


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            verdict = "MISSING in " + ("parent" if k not in a else "new")
        elif a[k] == b[k]:
            verdict = "IDENTICAL"
        elif region(a[k]) == region(b[k]):
            verdict = "PIPELINE"
        elif mfma_blocks(a[k]) and mfma_blocks(a[k]) == mfma_blocks(b[k]):
            verdict = "LOOPS"
        else:
            verdict = "DIFFERENT"
        bad += verdict not in ("IDENTICAL", "PIPELINE", "LOOPS")
        print(f"{verdict:10s} {k}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
