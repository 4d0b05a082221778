"""hipcc's kernel resource remarks (registers, LDS, scratch per kernel), as the host tests read them.  The compile that makes a
device unit's object for libmi355pt.so keeps what the compiler printed next to that object; `make asm-*` brings the objects of its units
up to date and prints those files.  So a report is about the code that ships, and no test compiles a unit the build already compiled."""
import os
import re
import shlex
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owl-path-tracer_amd", "csrc")
REMARKS = "-Rpass-analysis=kernel-resource-usage"
FIELDS = (("sgprs", r"TotalSGPRs: (\d+)"), ("vgprs", r"VGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))


def _make(*args, timeout):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    # (a CXXFLAGS of the caller's environment would override the Makefile's)
    env = {k: v for k, v in os.environ.items() if k not in ("CXXFLAGS", "MAKEFLAGS")}
    r = subprocess.run(["make", "-s", "-C", CSRC] + list(args), env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return r.stdout + r.stderr


def report(target):
    """`make <target>` (asm, asm-wt, asm-aov, ...): the report text, and (function name, VGPRs, scratch bytes per lane) of every kernel in it."""
    text = _make(target, timeout=1500)
    return text, re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S)


def resources(target):
    """{function name: {sgprs, vgprs, agprs, scratch, occupancy, lds}} of the same report."""
    blocks = re.findall(r"Function Name: (\S+)" + "".join(".*?" + pat for _, pat in FIELDS), report(target)[0], flags=re.S)
    assert len({b[0] for b in blocks}) == len(blocks)
    return {b[0]: {key: int(v) for (key, _), v in zip(FIELDS, b[1:])} for b in blocks}


def compile_command(unit):
    """The words of the command `make -n` prints for the object of <unit>.hip that libmi355pt.so is linked from."""
    dry = _make("-n", "-W", unit + ".hip", "build/product/%s.o" % unit, timeout=60)
    lines = [ln for ln in dry.splitlines() if " -c " in ln and unit + ".hip" in ln]
    assert len(lines) == 1, dry
    return shlex.split(lines[0])


def assert_ships_with_makefile_flags(unit):
    """The object is compiled for gfx950 with the Makefile's CXXFLAGS, in order, and with the remark flag: the report is that compile's."""
    with open(os.path.join(CSRC, "Makefile")) as f:
        flags = shlex.split(re.search(r"^CXXFLAGS\s*\?=(.*)$", f.read(), flags=re.M).group(1))
    made = compile_command(unit)
    assert made[:2] == [made[0], "--offload-arch=gfx950"] and made[2:2 + len(flags)] == flags and REMARKS in made and unit + ".hip" in made, (flags, made)
