"""The queue of deferred transfer callbacks (csrc/host/cbq.h) without a device: tests/c/cbq_sanitize.c
drives it with a clock in place of the GPU and checks FIFO order, exactly-once delivery, that no
callback runs before its fence, re-entry from a callback, and 80 entries through the capacity of
64. Built plain here; `make -f tests/c/cbq_sanitize.mk` runs the same program under
AddressSanitizer + UBSan. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_callback_queue_program(tmp_path):
    exe = str(tmp_path / "cbq")
    subprocess.run(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror",
                    "-I" + os.path.join(ROOT, "libplacebo_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "c", "cbq_sanitize.c"), "-o", exe],
                   check=True, capture_output=True, text=True, timeout=120)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
