"""The one helper that allocates and cuts a plan's device arrays (arena_alloc, csrc/host/arena.h), on the CPU:
tests/emu/arena_check.c is compiled with AddressSanitizer + UBSan against malloc-backed stand-ins for the two device
calls and run as a program of its own -- growth, a failed allocation, zero-byte parts, every slot on a multiple of 256
bytes and in order."""
import os
import subprocess

import harness


def test_arena_alloc_under_sanitizers(tmp_path):
    src = os.path.join(harness.REPO, "tests", "emu", "arena_check.c")
    out = str(tmp_path / "arena_check")
    subprocess.check_call(
        ["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-D_POSIX_C_SOURCE=200809L",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-I" + os.path.join(harness.REPO, "include"), "-I" + os.path.join(harness.REPO, "include", "compat"),
         "-I" + os.path.join(harness.REPO, "aws-c-compression_amd", "csrc", "host"), src, "-o", out])
    done = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert done.returncode == 0, (done.stdout + done.stderr)[-4000:]
    assert done.stdout.strip() == "arena ok"
