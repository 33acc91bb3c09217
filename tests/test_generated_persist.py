"""The committed persistent program (rlnc_amd/csrc/bitslice_jump_persist.inc) is exactly what gen_bsjump.py emits beside
bitslice_jump.inc with its default arguments (CPU, no device), and the host passes exactly the operands it names."""
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rlnc_amd", "csrc")


def test_persistent_inc_is_current(tmp_path):
    out = tmp_path / "bitslice_jump.inc"
    subprocess.check_call([sys.executable, os.path.join(CSRC, "gen_bsjump.py"), "--out", str(out)])
    with open(os.path.join(CSRC, "bitslice_jump_persist.inc"), "rb") as f:
        committed = f.read()
    assert (tmp_path / "bitslice_jump_persist.inc").read_bytes() == committed, \
        "bitslice_jump_persist.inc is stale: run `python gen_bsjump.py` in rlnc_amd/csrc"


def test_persistent_program_operands_are_the_hosts():
    text = open(os.path.join(CSRC, "bitslice_jump_persist.inc")).read()
    host = open(os.path.join(CSRC, "bsj_tile.hpp")).read()
    block = host[host.index("asm volatile(RLNC_BSJ_ASM_W8P"):]
    block = block[:block.index("RLNC_BSJ_CLOBBER_P")]
    passed = set(re.findall(r"\[(\w+)\] \"[sv]\"", block))
    used = set(re.findall(r"%\[(\w+)\]", text))
    assert used <= passed, sorted(used - passed)
    # an input the program never names still occupies a register of a kernel at the 256-VGPR limit (the second set-slot
    # base comes through RLNC_BSJ_P_BASE2_OPERANDS only where the program names it)
    assert passed <= used, sorted(passed - used)
    base2 = re.search(r"#define RLNC_BSJ_P_BASE2_OPERANDS(.*)\n", text).group(1)
    assert ("ldsc2" in base2) == bool({"ldsc2", "ldscw2"} & used)
    assert int(re.search(r"#define RLNC_BSJ_PERSIST_MIN_SOURCES (\d+)", text).group(1)) == 12
