"""The run-time to compile-time dispatchers of the sw2d launch layer (blitzdg_amd/csrc/hip/sw2d_dispatch.hpp) without a GPU:
tests/dispatch_check.cpp calls each with a recording callable for every mode in range and around it, both filter values and
every order from 0 to one past the maximum; compiled for the host with -fsanitize=address,undefined and run as a program of
its own. The (mode, filter) and order constants a dispatcher reaches are the kernel instances a per-order file compiles, so the
lists below are exact: one more is a kernel nobody asked for, one fewer a launch that fails at run time."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (-1, 0, 1, 2, 3, 4, 99)                       # as in dispatch_check.cpp
TRI = dict(RHS=0, LSERK=1, COMBINE=2)                 # StageMode (sw2d_kernels.hpp), CMODE_* (sw2d_curved_kernel.hpp)
QUAD = dict(RHS=0, COMBINE=1, LSERK=2, HEUN=3)        # QuadMode (sw2d_quad_kernel.hpp)

# dispatcher -> the (mode, filter) instances that exist
INSTANCES = {
    "forModeFilter": {(TRI[m], f) for m in ("RHS", "COMBINE") for f in (0, 1)} | {(TRI["LSERK"], 0)},
    "curvedForMode": {(m, f) for m in TRI.values() for f in (0, 1)},
    "quadForMode": {(QUAD[m], f) for m in ("RHS", "COMBINE") for f in (0, 1)} | {(QUAD["LSERK"], 0)},
    "quadForModeHeun": {(QUAD[m], f) for m in ("RHS", "COMBINE", "HEUN") for f in (0, 1)} | {(QUAD["LSERK"], 0)},
}


def expected_lines():
    """(dispatcher, arg, filter) -> the constants the callable is reached with, or None where the call is refused; in the
    program's order."""
    out = []
    for mode in MODES:
        out.append((("forMode", mode, 0), str(mode) if mode in TRI.values() else None))
        for filt in (0, 1):
            for name in ("forModeFilter", "curvedForMode", "quadForMode", "quadForModeHeun"):
                out.append(((name, mode, filt), f"{mode},{filt}" if (mode, filt) in INSTANCES[name] else None))
    for name, top in (("forOrder8", 8), ("forOrder12", 12)):
        for order in range(0, top + 2):
            out.append(((name, order, 0), str(order) if 1 <= order <= top else None))
    return out


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dispatch")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("no sanitizer runtime for g++ on this machine")
    exe = str(tmp / "dispatch_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "blitzdg_amd", "csrc", "hip"),
           os.path.join(ROOT, "tests", "dispatch_check.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600, cwd=str(tmp),
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert run.returncode == 0 and run.stdout.rstrip().endswith("dispatch ok"), run.stdout[-2000:] + run.stderr[-4000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    lines = run.stdout.splitlines()
    assert lines[0].startswith("invalid=")
    calls = []
    for text in lines[1:-1]:
        name, *fields = text.split()
        kv = dict(f.split("=", 1) for f in fields)
        calls.append(((name, int(kv["arg"]), int(kv["filter"])),
                      dict(ret=int(kv["ret"]), calls=int(kv["calls"]), passed=int(kv["passed"]), reached=kv["reached"])))
    return int(lines[0].split("=")[1]), calls


def test_every_call_was_made_once_in_order(report):
    _, calls = report
    assert [key for key, _ in calls] == [key for key, _ in expected_lines()]


def test_the_instances_reached_are_exactly_the_compiled_ones(report):
    _, calls = report
    got = {key: r["reached"] for key, r in calls if r["calls"]}
    want = {key: reached for key, reached in expected_lines() if reached is not None}
    assert got == want
    # the sets of the issue, spelled out: five straight instances, six curved, five / seven quadrilateral, three plain modes
    count = lambda name: sum(1 for key in got if key[0] == name)
    assert [count(n) for n in ("forMode", "forModeFilter", "curvedForMode", "quadForMode", "quadForModeHeun", "forOrder8", "forOrder12")] \
        == [3, 5, 6, 5, 7, 8, 12]


def test_an_accepted_call_runs_the_callable_once_and_returns_its_answer(report):
    invalid, calls = report
    want = dict(expected_lines())
    for key, r in calls:
        if want[key] is not None:
            assert r["calls"] == 1 and r["passed"] == 1 and r["ret"] != invalid, (key, r)


def test_everything_else_is_an_invalid_value(report):
    invalid, calls = report
    want = dict(expected_lines())
    refused = [(key, r) for key, r in calls if want[key] is None]
    assert len(refused) == len(calls) - (3 + 5 + 6 + 5 + 7 + 8 + 12)
    for key, r in refused:
        assert r["calls"] == 0 and r["ret"] == invalid and r["reached"] == "", (key, r)
