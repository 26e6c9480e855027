"""TEST INFRASTRUCTURE.  The fit kernel (fit_kernels.hip) against the emulator build of the library made with
AddressSanitizer on top of UBSan (tests/test_emulated_fit_asan.py builds it and runs this with libasan preloaded): every
count vector under every pair of bounds, lengths and tables against the host's, with every access of the kernel's code --
the lists in LDS, the two tables in device memory -- checked."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fit_api as fa  # noqa: E402
import harness  # noqa: E402

lib = fa.bind(harness.load_product(sys.argv[1]))
engines = [fa.FittedEngine(lib, lo, hi) for lo, hi in fa.BOUNDS]
fa.run_lengths_equal_host(lib, engines)
fa.run_tables_equal_host(lib, engines)
for e in engines:
    e.close()
print("no finding")
