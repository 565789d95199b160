"""The thread-safe containers of the file dispatchers (otter_amd/csrc/otg_dispatch_queue.hpp: BoundedQueue, OrderedOutput) on the CPU under
ThreadSanitizer.  tests/dispatch_queue_driver.cpp includes only that header and covers: several threads delivering batches out of order to
one writer with a cap smaller than the number of batches (the writer sees 0..n-1 in order, never more than cap held back plus the one the
writer takes next); the batch the writer wants arriving last; a failure raised while producers are blocked on a full output and the writer
on a missing batch; BoundedQueue finish with items still queued, and abort.  Pass = exit 0 and no sanitizer report.

The compiler is ROCm's clang++ where it exists, else g++.  (The waiters poll with condition_variable::wait_for, which is
pthread_cond_clockwait underneath; the libtsan of GCC 11 does not intercept that call and reports the mutex it releases as locked twice.
A g++ whose TSan run of a bare wait_for is not clean is therefore treated as a compiler without TSan.)"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "dispatch_queue_driver.cpp")
CSRC = os.path.join(ROOT, "otter_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=thread", "-pthread"]
# a hang detector only: the driver needs about half a second (its own watchdog gives up after 30 s)
DRIVER_TIMEOUT_S = 120
PROBE = """#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
int main() {
  std::mutex m; std::condition_variable cv; bool go = false;
  std::thread t([&] { std::unique_lock<std::mutex> lk(m); while (!go) cv.wait_for(lk, std::chrono::milliseconds(5)); });
  std::this_thread::sleep_for(std::chrono::milliseconds(30));
  { std::lock_guard<std::mutex> lk(m); go = true; }
  t.join();
}
"""


def _tsan_compiler(tmp):
    """the first compiler that builds the probe with -fsanitize=thread and runs it without a report"""
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write(PROBE)
    for cxx in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")):
        if not cxx or not os.path.exists(cxx):
            continue
        exe = os.path.join(tmp, "probe_" + os.path.basename(cxx))
        if subprocess.run([cxx] + FLAGS + ["-o", exe, src], capture_output=True).returncode != 0:
            continue
        r = subprocess.run([exe], capture_output=True, timeout=DRIVER_TIMEOUT_S)
        if r.returncode == 0 and b"ThreadSanitizer" not in r.stderr:
            return cxx
    return None


def test_dispatch_queue_under_tsan(tmp_path):
    cxx = _tsan_compiler(str(tmp_path))
    if cxx is None:
        pytest.skip("no compiler with a working ThreadSanitizer")
    exe = str(tmp_path / "dispatch_queue_driver")
    subprocess.check_call([cxx] + FLAGS + ["-I" + CSRC, "-o", exe, DRIVER])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=DRIVER_TIMEOUT_S)
    print(r.stdout[-2000:], r.stderr[-4000:])
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    assert r.stdout.strip().endswith("ok")
