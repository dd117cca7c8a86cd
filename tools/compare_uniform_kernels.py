#!/usr/bin/env python
"""No-GPU check that a change leaves the existing kernels alone: compile the given .hip files of two source trees to gfx950
device assembly and compare, kernel by kernel, the instruction streams of every kernel the OLD tree has.

    python tools/compare_uniform_kernels.py OLD_TREE [NEW_TREE] [file.hip ...]

The ragged forms are instantiations of the uniform kernels' templates with a trailing parameter pack (empty in the uniform
instantiations), so a uniform kernel's mangled name gains an empty pack ("J E" in the template arguments, "DpT<n>_" in the
parameter list); names are compared with that removed -- also where the pack is the ONLY template parameter, i.e. the old
tree's kernel was not a template at all (a template's own name is a substitution candidate of its mangled name, so the
S<n>_ back-references of its parameter list are shifted back by one).  Labels are renumbered; comments and directives are dropped."""
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ["srf_encoder.hip", "srf_elementwise.hip", "srf_pyramid.hip", "srf_pyramid_reg.hip", "srf_pwconv_x3w.hip", "srf_pwconv_x3f.hip",
           "srf_tac.hip", "srf_pwconv_small.hip"]


_B36 = "0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZ"


def _unshift(m):
    """A template's name is the first substitution candidate of its mangled name, a plain function's is not: S_ / S0_ / S1_ ...
    in the parameter list of the templated form are S<one less>_ in the plain form (base-36 sequence ids, S_ before S0_)."""
    seq = m.group(1)
    if seq == "":
        return m.group(0)                                                      # (the template itself: not in a parameter list)
    n = int(seq, 36) - 1
    if n < 0:
        return "S_"
    digits = ""
    while True:
        digits = _B36[n % 36] + digits
        n //= 36
        if not n:
            return "S%s_" % digits


def kernels(asm):
    out, cur, name = {}, None, None
    for line in open(asm, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        t = line.split(";")[0].strip()
        if t.startswith(".Lfunc_end"):
            key = re.sub(r"JE(E.*?)DpT\d*_$", r"\1", name)
            if key != name and "IEv" in key:                                   # (a plain kernel that became a template: "I E v")
                head, tail = key.split("IEv", 1)
                key = head + re.sub(r"S([0-9A-Z]*)_", _unshift, tail)
            out[key] = cur
            cur = None
        elif t.startswith(".LBB"):
            cur.append(re.sub(r"\d+_", "_", t))
        elif t and not t.startswith("."):
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
    return out


def assemble(tree, src, tmp, tag):
    sys.path.insert(0, HERE)
    from sudo_rm_rf_amd import build as b          # (the flags of THIS tree for both)
    out = os.path.join(tmp, "%s_%s.s" % (tag, src))
    cmd = [b.hipcc()] + b.FLAGS + b.FILE_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(tree, "sudo_rm_rf_amd", "csrc", src), "-o", out]
    subprocess.run(cmd, check=True, capture_output=True)
    return out


def main(argv):
    if not argv:
        sys.exit(__doc__)
    old = argv[0]
    new = argv[1] if len(argv) > 1 and os.path.isdir(argv[1]) else HERE
    files = [a for a in argv[1:] if a.endswith(".hip")] or DEFAULT
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        for src in files:
            a, b = kernels(assemble(old, src, tmp, "old")), kernels(assemble(new, src, tmp, "new"))
            for k in sorted(a):
                if "9SrfFrames" in k and k not in b:          # a ragged form whose table arguments changed: not a uniform kernel
                    print("%-22s %s %s" % (src, "ragged   ", k))
                    continue
                same = k in b and a[k] == b[k]
                bad += not same
                print("%-22s %s %s" % (src, "same     " if same else ("MISSING  " if k not in b else "DIFFERENT"), k))
            print("%-22s %d kernels only in the new tree" % (src, len(set(b) - set(a))))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main(sys.argv[1:])
