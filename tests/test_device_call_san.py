"""CPU: the block layout of csrc/device_call.hpp under AddressSanitizer and UndefinedBehaviorSanitizer.

A stand-alone program (tests/cpp/device_call_main.cpp, its own main) includes the header without HIP and lays out
request lists over malloc'ed blocks of exactly `need` bytes: parts of 0, 1, 255, 256 and 257 bytes, parts that are
not needed, element types of 1, 4, 8 and 16 bytes, and the triangulate- and pose-shaped lists with host and with
device inputs, each against the sums that the entry points' hand-kept size lists gave.  It writes every byte of
every part.  It runs as a child process and must exit clean.  The sanitizer runtimes are linked into the program, so
it needs nothing from the environment it is started in.  Fails without the feature: the header does not exist."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_layout_under_sanitizers(tmp_path):
    exe = tmp_path / "device_call_main"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    os.path.join(REPO, "tests", "cpp", "device_call_main.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ""
    assert r.stdout == "ok 13\n"
