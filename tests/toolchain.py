"""The compiler invocations the CPU tests share: a host build of kernel text behind a stub <hip/hip_runtime.h>, as a shared library or as a
stand-alone program (plain or under the address and undefined-behaviour sanitizers), and the gfx950 assembly listing of a .hip file with its
kernels' resource fields. None needs a GPU; a test is skipped where the compiler is absent."""
import collections
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "icepy4d_amd", "csrc")
CLANGXX = "/opt/rocm/llvm/bin/clang++"
HIPCC = "/opt/rocm/bin/hipcc"
HIP_STUB = "#pragma once\n#define __device__\n#define __forceinline__ inline\n"


def host_library(tmp_dir, harness_cpp):
    """tests/<harness_cpp> and the csrc headers it includes as a shared library: the very text the kernels compile, with __device__ and
    __forceinline__ defined away and contraction off (the headers that matter switch it off themselves; the flag covers the rest)."""
    if not os.path.exists(CLANGXX):
        pytest.skip("no clang++")
    os.makedirs(os.path.join(tmp_dir, "hip"), exist_ok=True)
    with open(os.path.join(tmp_dir, "hip", "hip_runtime.h"), "w") as f:
        f.write(HIP_STUB)
    so = os.path.join(tmp_dir, "lib" + os.path.splitext(os.path.basename(harness_cpp))[0] + ".so")
    r = subprocess.run([CLANGXX, "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + str(tmp_dir), "-I" + CSRC,
                        os.path.join(ROOT, "tests", harness_cpp), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return ctypes.CDLL(so)


def host_program(tmp_dir, harness_cpp, sanitize):
    """tests/<harness_cpp>, which has a main of its own, and the csrc headers it includes as a stand-alone program, built plain or with the
    address and undefined-behaviour sanitizers: the path of the executable. The sanitizer runtimes are asked for with an empty program
    before the harness is built, so the harness's own failure to build is never a skip."""
    if not os.path.exists(CLANGXX):
        pytest.skip("no clang++")
    tmp_dir = str(tmp_dir)
    os.makedirs(os.path.join(tmp_dir, "hip"), exist_ok=True)
    with open(os.path.join(tmp_dir, "hip", "hip_runtime.h"), "w") as f:
        f.write(HIP_STUB)
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"] if sanitize else ["-O2"]
    if sanitize:
        probe = os.path.join(tmp_dir, "sanitizer_probe.cpp")
        with open(probe, "w") as f:
            f.write("int main() { return 0; }\n")
        r = subprocess.run([CLANGXX, *flags, probe, "-o", os.path.join(tmp_dir, "sanitizer_probe")], capture_output=True, text=True)
        if r.returncode != 0:
            pytest.skip("this clang++ has no sanitizer runtimes")
    exe = os.path.join(tmp_dir, os.path.splitext(os.path.basename(harness_cpp))[0] + ("_san" if sanitize else ""))
    r = subprocess.run([CLANGXX, "-std=c++17", "-ffp-contract=off", *flags, "-I" + tmp_dir, "-I" + CSRC, os.path.join(ROOT, "tests", harness_cpp), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def device_listing(hip_file, tmp_dir):
    """The gfx950 assembly of csrc/<hip_file> (device side only), as text."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    out = os.path.join(tmp_dir, os.path.splitext(hip_file)[0] + ".s")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(CSRC, hip_file), "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read()


def kernel_resources(text):
    """{kernel symbol: {field: int}} out of the metadata of a listing: vgpr_count, vgpr_spill_count, sgpr_spill_count,
    private_segment_fixed_size, ... Where a field is named more than once in an entry (its arguments have .size and .offset of their own) the
    first one counts; a field the entry lacks reads 0."""
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        fields = collections.defaultdict(int)
        for k, v in re.findall(r"\.(\w+):[ \t]+(\d+)[ \t]*$", blk, re.M):
            fields.setdefault(k, int(v))
        out[re.search(r"\.name:\s+(\S+)", blk).group(1)] = fields
    return out


def kernel_body(text, symbol):
    """The instructions of one kernel: from its label to the end of the function."""
    body = text[text.index(symbol + ":"):]
    return body[:body.index(".Lfunc_end")]
