"""csrc/session_slots.h — the slot ledger, the slot-list check and the penalty table the sessions of all three models share — built with the
host compiler alone (no HIP) under AddressSanitizer and UBSan, and run as a child process: tests/session_slots_main.cpp holds the checks and
exits non-zero at the first that fails.  Where a sanitized program does not link or start, the same program is built and run without the flag."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "session_slots_main.cpp")
HEADER = os.path.join(ROOT, "tts.cpp_amd", "csrc", "session_slots.h")
# what the dynamic loader or a sanitizer runtime prints when the program cannot start on this host (none of them is a finding in the program)
NO_START = ("error while loading shared libraries", "runtime does not come first in initial library list", "ReserveShadowMemoryRange failed",
            "Shadow memory range interleaves", "LeakSanitizer has encountered a fatal error")


def _build(cxx, exe, sanitize):
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else [])
    return subprocess.run(cmd + [SRC, "-o", exe], capture_output=True, text=True)


def test_header_has_no_hip_in_it():
    text = open(HEADER).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert sorted(includes) == ["<math.h>", "<stdint.h>", "<vector>"], includes
    assert "int set_err(const char *fmt, ...);" in text


def test_slot_ledger_list_check_and_penalty_table(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    if cxx is None:
        pytest.fail("no host C++ compiler (c++ / g++)")
    exe = str(tmp_path / "session_slots_main")
    built = _build(cxx, exe, sanitize=True)
    ran = subprocess.run([exe], capture_output=True, text=True) if built.returncode == 0 else None
    # unusable: the sanitized program does not link, or the loader / the runtime's start-up says it cannot run here.  Any other non-zero exit
    # (a failed check, or a report of any sanitizer) is a failure
    sanitizer_unusable = built.returncode != 0 or (ran.returncode != 0 and any(m in ran.stderr for m in NO_START))
    if sanitizer_unusable:   # the checks themselves still run
        built = _build(cxx, exe, sanitize=False)
        assert built.returncode == 0, built.stderr
        ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "session_slots: ok" in ran.stdout
