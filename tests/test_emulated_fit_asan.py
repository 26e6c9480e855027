"""The fit kernel compiled for the CPU with AddressSanitizer + UBSan (GPU sanitizers are not available on the pool): the
scenarios of test_device_lengths_equal_host_lengths and test_device_tables_equal_host_engine_tables (tests/test_emulated_fit.py)
with every load and store of the kernel checked.  The build is the one tests/test_emulated_asan.py makes, in the same place."""
import os
import subprocess
import sys
import tempfile

import harness

EMU_DIR = os.path.join(harness.REPO, "tests", "emu")
BUILD = os.path.join(tempfile.gettempdir(), "aws-c-compression-emu-asan-%d" % os.getuid())
ASAN_SO = os.path.join(BUILD, "libaws-c-compression-emu-asan.so")


def test_fit_under_address_sanitizer():
    subprocess.check_call(
        ["make", "-s", "-C", EMU_DIR, "BUILD=" + BUILD, "TARGET=" + ASAN_SO,
         "SAN=-fsanitize=address,undefined -fno-sanitize-recover=undefined"], stdout=subprocess.DEVNULL)
    libasan = subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip()
    # (the emulator's work-items are ucontext fibers: the stack-use-after-return mode does not know them)
    env = dict(os.environ, LD_PRELOAD=libasan, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    done = subprocess.run([sys.executable, os.path.join(EMU_DIR, "fit_asan_driver.py"), ASAN_SO], env=env, capture_output=True,
                          text=True, timeout=1200)
    assert done.returncode == 0, (done.stdout + done.stderr)[-4000:]
    assert "no finding" in done.stdout
