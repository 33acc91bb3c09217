"""CPU: the host copy pool (rlnc_amd/csrc/host_copy.cpp) on unaligned destinations and odd lengths, as a stand-alone
program (tests/cpp/test_host_copy.cpp) -- built plain, with the address sanitizer and with the thread sanitizer, and
run.  No device call is made and nothing here is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.parametrize("sanitizer", [None, "address", "thread"])
def test_host_copy_program(tmp_path, sanitizer):
    exe = tmp_path / "test_host_copy"
    # host_copy.cpp as plain host C++ (the HIP headers only declare); what it references outside itself -- the engine's
    # error string and the HIP entry points of copy_out, which the program never calls -- comes from
    # tests/cpp/host_copy_stubs.cpp, so no HIP library is linked
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
           os.path.join(ROOT, "rlnc_amd", "csrc", "host_copy.cpp"),
           os.path.join(ROOT, "tests", "cpp", "host_copy_stubs.cpp"),
           os.path.join(ROOT, "tests", "cpp", "test_host_copy.cpp"), "-pthread", "-o", str(exe)]
    if sanitizer:
        cmd[4:4] = ["-fsanitize=" + sanitizer, "-fno-omit-frame-pointer"]
    subprocess.check_call(cmd)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "host copy pool ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
