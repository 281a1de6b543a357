"""Native runtime under ThreadSanitizer: the shm SPSC ring's producer and
consumer threads move variable-size records through a small ring (constant wrap-around)."""
import os
import platform
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixed_layout_prefix():
    """ThreadSanitizer's runtime aborts at start-up ("unexpected memory mapping") where the kernel
    randomises mappings over more address bits than the runtime's shadow layout allows
    (vm.mmap_rnd_bits above 28 with the gcc 11 runtime), so the instrumented program runs with
    address randomisation off for that one process (``setarch -R``).  Returns the command prefix:
    empty where the kernel's setting needs none, None where it does and the prefix is refused."""
    if shutil.which("setarch"):
        pre = ["setarch", platform.machine(), "-R"]
        if subprocess.run(pre + ["true"], capture_output=True).returncode == 0:
            return pre
    try:
        with open("/proc/sys/vm/mmap_rnd_bits") as f:
            bits = int(f.read())
    except (OSError, ValueError):
        return []
    return [] if bits <= 28 else None


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("sanitize", ["thread", None])
def test_ring_stress(tmp_path, sanitize):
    pre = _fixed_layout_prefix() if sanitize else []
    if pre is None:
        pytest.skip("ThreadSanitizer cannot start here: vm.mmap_rnd_bits is above 28 and this system "
                    "refuses to turn address randomisation off for one process (setarch -R)")
    exe = str(tmp_path / "ring_stress")
    cmd = ["g++", "-std=c++17", "-O1", "-g", os.path.join(REPO, "csrc/runtime/shm_ring.cpp"),
           os.path.join(REPO, "csrc/runtime/tests/ring_stress.cpp"), "-o", exe, "-lrt", "-lpthread"]
    if sanitize:
        cmd.insert(1, f"-fsanitize={sanitize}")
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and sanitize and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime unavailable")
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([*pre, exe, "5000"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "OK 5000 records" in p.stdout, p.stderr[-3000:]
    assert "WARNING: ThreadSanitizer" not in p.stderr
