"""The gfx950 device assembly of a translation unit exactly as csrc/Makefile compiles it (`make build/<tu>.s`: the library's own
FLAGS plus -S --cuda-device-only), and the three cuts the ISA tests of test_host_logic.py make in that text."""
import os
import re
import shutil
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "danbo-pytorch_amd", "csrc")


def device_asm(tu):
    """text of build/<tu>.s; make compiles it once and again only after a source or header changed"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-C", CSRC, "HIPCC=" + hipcc, "build/%s.s" % tu], check=True, capture_output=True)
    return open(os.path.join(CSRC, "build", tu + ".s")).read()


def kernel_body(text, pattern):
    """the lines from the label of the kernel whose mangled name matches `pattern` (a regex, or the full name) to its .Lfunc_end"""
    body = text[text.index(re.search(r"^(" + pattern + r"):", text, re.M).group(1) + ":"):]
    return body[:body.index(".Lfunc_end")].split("\n")


def kernel_meta(text, pattern, field):
    """the regex match (group 1: the integer) of metadata field `field` of the kernel whose .name matches `pattern`, or None"""
    return re.search(r"\.name:\s+" + pattern + r"\n(?:.*\n)*?\s+\." + field + r":\s+(\d+)", text)


def asm_lines(body):
    """(inside inline asm?, line) for every line of a body; an ASMSTART marker counts as inside, an ASMEND marker as outside.
    The marker lines themselves are yielded too (two of the tests used to step over them): they are comments, `;;#ASMSTART` /
    `;;#ASMEND`, with nothing in front of the `;`, so no check of an instruction or a register can match one."""
    in_asm = False
    for l in body:
        in_asm = True if "ASMSTART" in l else (False if "ASMEND" in l else in_asm)
        yield in_asm, l
