"""Emit build/build_info.cpp: dd_build_info() returns the ABI version, the
sha256 of the device ISA of the step translation unit (step.hip) and of the
fused policy rollout, and of the step and rollout kernels' own function bodies
(step_kernel_isa from step.s, rollout_kernel_isa from rollout.s), so a counter
summary can be tied to the exact code it was measured on (bench.py compares
the row's kernel hash before reporting roofline.traffic /
rollout_point.traffic).

    python tools/build_info.py step.s rollout.s policy_rollout.s [step_fast.s] > build_info.cpp

With step_fast.s (the headline shape's own kernel, csrc/step_fast.hip) the
string also carries step_fast_kernel_isa, so a counter row of that kernel is
tied to its code and not to the generic step kernels'."""
import hashlib
import re
import sys


def digest(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for line in f:
            if line.lstrip().startswith((b";", b"//")):  # comments only; every instruction and directive counts
                continue
            h.update(line)
    return h.hexdigest()[:16]


_LABEL_NO = re.compile(rb"\.(LBB|LCPI|Lfunc_end|Ltmp)\d+")
# e.g. a block label's "; in Loop: Header=BB<f>_<b>": the function number again
_TRAILING_COMMENT = re.compile(rb"\s*;.*$")


def kernel_digest(path: str, prefix: bytes) -> str:
    """sha256 of the bodies of every function whose symbol starts with
    `prefix` (from its `sym:` label to its `.Lfunc_end` label), comments
    skipped: a change elsewhere in the translation unit leaves it alone, so
    a PMC row of one kernel stays valid across edits of the others.  Label
    numbers that count the functions before it (.LBB<f>_<b>, .Lfunc_end<f>,
    .Ltmp<k>, .LCPI<f>_<k>) are normalised and the comments after an
    instruction or label (which repeat those numbers) dropped for the same
    reason, so the hash follows a kernel from one unit to another.  A prefix that
    matches no function is an error: the hash of nothing would stay equal to
    itself across every later edit."""
    h = hashlib.sha256()
    inside = False
    found = 0
    with open(path, "rb") as f:
        for line in f:
            if not inside and line.startswith(prefix) and line.split(None, 1)[0].endswith(b":"):
                inside = True
                found += 1
            if inside:
                if line.lstrip().startswith((b";", b"//")):
                    continue
                h.update(_TRAILING_COMMENT.sub(b"", _LABEL_NO.sub(rb".\1", line)))
                if line.startswith(b".Lfunc_end"):
                    inside = False
    if not found:
        raise ValueError(f"{path}: no function starts with {prefix.decode()}")
    return h.hexdigest()[:16]


def main(step_isa: str, rollout_isa: str, policy_rollout_isa: str, step_fast_isa: str = "") -> None:
    info = (f";step_isa={digest(step_isa)};policy_rollout_isa={digest(policy_rollout_isa)}"
            f";step_kernel_isa={kernel_digest(step_isa, b'_ZN2dd11step_kernel')}"
            f";rollout_kernel_isa={kernel_digest(rollout_isa, b'_ZN2dd14rollout_kernel')}")
    if step_fast_isa:
        info += f";step_fast_kernel_isa={kernel_digest(step_fast_isa, b'_ZN2dd16step_fast_kernel')}"
    print('#include "dronestep.h"')
    print("#define DD_STR2(x) #x")
    print("#define DD_STR(x) DD_STR2(x)")
    print(f'extern "C" const char* dd_build_info(void) {{ return "abi=" DD_STR(DD_ABI_VERSION) "{info}"; }}')


if __name__ == "__main__":
    main(*sys.argv[1:5])
