"""The policy of the preview chain (csrc/library/preview_state.h) on the CPU: tests/native/preview_state_main.cpp is a stand-alone
program, built here with AddressSanitizer + UBSan and run directly.  It is fed the table of tests/preview_refusals.py -- every state, every
preview call, every bad argument that preview_state.h has a word on -- and must answer each line with the recorded code and message, byte
for byte; it also checks what each event keeps and empties (the rules tests/test_history.py::test_states_and_error_codes states)."""
import os
import shutil
import subprocess

import pytest

from tests import preview_refusals as table
from tests.conftest import ROOT


def test_preview_state_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "preview_state_main")
    inc = os.path.join(ROOT, "raytracingincuda_amd", "csrc", "library")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + inc, "-o", exe, os.path.join(ROOT, "tests", "native", "preview_state_main.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [(s, c, varied, args) for s, c, varied, args in table.cases() if varied not in table.OWN_PARAMETERS]
    assert len(cases) > 2000 and {c for _, c, _, _ in cases} == set(table.CALLS)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=66", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input="".join(table.program_line(s, c, args) + "\n" for s, c, _, args in cases), capture_output=True, text=True, env=env)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    answers = r.stdout.splitlines()
    assert answers[-1] == "0 preview-state rule failure(s)" and len(answers) == len(cases) + 1
    want = table.expected()
    wrong = []
    for (s, c, varied, args), answer in zip(cases, answers):
        code, message = answer.split(" | ", 1) if " | " in answer else (answer.rstrip(" |"), "")
        if (int(code), message) != want[(s, c, table.label(varied, args))]:
            wrong.append((s, c, table.label(varied, args), answer, want[(s, c, table.label(varied, args))]))
    assert not wrong, (len(wrong), wrong[:10])
