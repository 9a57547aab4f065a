"""hlynr_intercept_amd/build.py's control flow, no compiler involved: subprocess.check_call is replaced by a fake that writes the file
after `-o`, and every path the build writes (libraries, sidecars, lock, objects) is redirected into tmp_path."""
import os
import subprocess
import sys
import threading
import time

import pytest


@pytest.fixture
def fake_build(monkeypatch, tmp_path):
    """build.py with its outputs in tmp_path and a hot-word check that passes; returns (build, calls)."""
    from hlynr_intercept_amd import build, hotcheck
    calls = []

    def fake(cmd, cwd=None):
        calls.append(cmd)
        open(cmd[cmd.index("-o") + 1], "w").write("x")

    monkeypatch.setattr(build, "_HERE", str(tmp_path))
    monkeypatch.setattr(build, "LIB", str(tmp_path / "libhlx.so"))
    monkeypatch.setattr(build, "SAFE_LIB", str(tmp_path / "libhlx_safe.so"))
    monkeypatch.setattr(build, "LOCK", str(tmp_path / "libhlx.so.lock"))
    monkeypatch.setattr(build, "generate_baked", lambda verbose=False: "")
    monkeypatch.setattr(build, "write_inst_list", lambda insts, verbose=False: False)
    monkeypatch.setattr(build.subprocess, "check_call", fake)
    monkeypatch.setattr(hotcheck, "verify", lambda path=None: 1)
    for var in ("HLX_SINGLE_TU", "HLX_SAFE_BUILD", "HLX_LIBRARY", "MAX_JOBS"):
        monkeypatch.delenv(var, raising=False)
    return build, calls


def test_build_falls_back_to_the_safe_variant_when_the_lint_refuses(fake_build, monkeypatch):
    """A HotcheckViolation on the product build is answered with a second compilation carrying -DHLX_HOT_FROM_MEMORY=1, which is
    not linted for hot words, and leaves the marker file."""
    from hlynr_intercept_amd import hotcheck
    build, calls = fake_build
    lib = build.LIB

    def fake_verify(path=None):
        raise hotcheck.HotcheckViolation("hotcheck: the register allocator spilled a hot-constant register (test)")

    monkeypatch.setattr(hotcheck, "verify", fake_verify)
    monkeypatch.setenv("HLX_SINGLE_TU", "1")          # (one compiler call per library: the parallel path is test_parallel_build... below)
    assert build.build(force=True) == lib
    assert len(calls) == 2 and "-DHLX_HOT_FROM_MEMORY=1" not in calls[0] and "-DHLX_HOT_FROM_MEMORY=1" in calls[1]
    assert os.path.exists(lib) and os.path.exists(lib + ".safe") and os.path.exists(lib + ".rejected") and os.path.exists(lib + ".srchash")
    # ... and a clean product build afterwards removes the marker
    monkeypatch.setattr(hotcheck, "verify", lambda path=None: 1)
    calls.clear()
    assert build.build(force=True) == lib and len(calls) == 1 and not os.path.exists(lib + ".safe")


def test_parallel_build_splits_the_instantiations_and_falls_back_to_one_translation_unit(fake_build, monkeypatch):
    """One host unit + PARTS part units compiled with the TU macros and linked; a failure there is answered with the single
    translation unit; the list of instantiations is a pure function of a listing."""
    build, calls = fake_build
    lib = build.LIB
    assert build._listed() >= 80                                   # the committed hint file names the shipped instantiations
    assert build.build(force=True) == lib
    units = [c for c in calls if "-c" in c]
    assert len(units) == build.PARTS + 1 and sum("-DHLX_TU_HOST" in c for c in units) == 1
    assert sorted(d for c in units for d in c if d.startswith("-DHLX_TU_PART=")) == sorted(f"-DHLX_TU_PART={k}" for k in range(build.PARTS))
    assert len(calls) == build.PARTS + 2 and "-shared" in calls[-1] and all("-shared" not in c for c in units)
    # a compiler that fails on the split units: one translation unit, as in rounds 1-4
    calls.clear()

    def flaky(cmd, cwd=None):
        calls.append(cmd)
        if any(d.startswith("-DHLX_TU_PART=") for d in cmd):
            raise build.subprocess.CalledProcessError(1, cmd)
        open(cmd[cmd.index("-o") + 1], "w").write("x")

    monkeypatch.setattr(build.subprocess, "check_call", flaky)
    assert build.build(force=True) == lib and "-shared" in calls[-1] and not any(d.startswith("-DHLX_TU") for d in calls[-1])
    text = "<_ZN12_GLOBAL__N_114hlx_env_kernelILj608ELi0ELb0ELb0ELi2ELi1EEEvP>:\n<_ZN12_GLOBAL__N_114hlx_env_kernelILj639ELi1ELb1ELb0ELi0ELi0EEEvP>:"
    assert build.instantiations(text) == [(608, 0, 0, 0, 2, 1), (639, 1, 1, 0, 0, 0)]


def test_every_build_compiles_with_the_same_base_flags_and_links_with_z_defs(fake_build):
    """Product, safe (full and minimal) and stamps builds: every compilation of hlx_kernels.hip is FLAGS plus defines, `-c` or the
    link flags, and `-o`; every link refuses undefined symbols."""
    build, calls = fake_build
    build.build(force=True, with_safe=True)
    build.build_safe(force=True, minimal=True)
    build.build_stamps(2)
    compiles = [c for c in calls if c[-1] == build.SOURCE]
    links = [c for c in calls if "-shared" in c]
    assert len(compiles) == 2 * (build.PARTS + 1) + 2 and len(links) == 4
    assert all("-Wl,-z,defs" in c for c in links)
    defines = set()
    for c in compiles:
        assert c[1:1 + len(build.FLAGS)] == build.FLAGS, c
        rest = c[1 + len(build.FLAGS):-1]
        out = rest.index("-o")
        rest = rest[:out] + rest[out + 2:]
        assert ("-c" in rest) != ("-shared" in rest), c
        assert all(a.startswith("-D") or a in ["-c"] + build.LINK for a in rest), c
        defines.add(tuple(a for a in rest if a.startswith("-D") and not a.startswith("-DHLX_TU_")))
    assert defines == {(), tuple(build.SAFE_FLAGS), tuple(build.SAFE_FLAGS) + ("-DHLX_AB_MINIMAL",), ("-DHLX_STAMPS=2",)}


@pytest.mark.parametrize("max_jobs, limit", [(None, 16), ("3", 3)])
def test_both_libraries_share_one_pool_of_at_most_16_compilers(fake_build, monkeypatch, max_jobs, limit):
    build, calls = fake_build
    if max_jobs:
        monkeypatch.setenv("MAX_JOBS", max_jobs)
    monkeypatch.setattr(build.os, "cpu_count", lambda: 256)       # a large host does not raise the limit
    guard, now, peak = threading.Lock(), [0], [0]

    def slow(cmd, cwd=None):
        with guard:
            now[0] += 1
            peak[0] = max(peak[0], now[0])
        time.sleep(0.2)
        open(cmd[cmd.index("-o") + 1], "w").write("x")
        with guard:
            now[0] -= 1

    monkeypatch.setattr(build.subprocess, "check_call", slow)
    build.build(force=True, with_safe=True)
    assert peak[0] == limit          # 18 units: more than one library's worth in flight at once, never more than the limit


def test_headers_are_written_before_the_first_compile_and_after_the_last(fake_build, monkeypatch):
    """Under the lock: baked header, one hash, compile, hot-word check, rename, sidecars from that hash, instantiation list last.
    No generated header changes while a compiler may be reading it, and both sidecars describe what was compiled."""
    from hlynr_intercept_amd import hotcheck
    build, calls = fake_build
    events = []

    def fake(cmd, cwd=None):
        events.append("start")
        open(cmd[cmd.index("-o") + 1], "w").write("x")
        events.append("end")

    monkeypatch.setattr(build, "generate_baked", lambda verbose=False: events.append("baked"))
    monkeypatch.setattr(build, "write_inst_list", lambda insts, verbose=False: events.append("inst"))
    monkeypatch.setattr(hotcheck, "listing", lambda path=None: "")
    monkeypatch.setattr(build.subprocess, "check_call", fake)
    build.build(force=True, with_safe=True)
    assert events[0] == "baked" and events[-1] == "inst" and events.count("baked") == events.count("inst") == 1
    assert events.count("start") == events.count("end") == 2 * (build.PARTS + 2)
    h = open(build.LIB + ".srchash").read().split()
    assert h == [build._src_hash()] and open(build.SAFE_LIB + ".srchash").read().split() == h + ["full"]
    # up to date now: neither a second build nor a minimal safe build compiles anything
    events.clear()
    assert not build.needs_build() and build.safe_lib_variants() == "full"
    build.build(with_safe=True)
    build.build_safe(minimal=True)
    assert events == []


def test_src_hash_leaves_out_the_instantiation_list(monkeypatch, tmp_path):
    """hlx_inst_gen.h says where an instantiation is compiled, not what exists: rewriting it after a build leaves the build current."""
    import shutil
    from hlynr_intercept_amd import build
    csrc = str(tmp_path / "csrc")
    shutil.copytree(build.CSRC, csrc)
    monkeypatch.setattr(build, "CSRC", csrc)
    before = build._src_hash()
    with open(os.path.join(csrc, "hlx_inst_gen.h"), "a") as f:
        f.write("#if !defined(HLX_TU_PART) || HLX_TU_PART == 0\nHLX_INST(1u, 0, false, false, 0, 0)\n#endif\n")
    assert build._src_hash() == before
    with open(os.path.join(csrc, "hlx_kcfg.h"), "a") as f:
        f.write("// changed\n")
    assert build._src_hash() != before


def test_build_safe_waits_for_the_lock_and_then_finds_the_library_built(fake_build):
    """While another process holds the build lock, build_safe() compiles nothing; once that process has built the safe library and
    released the lock, build_safe() sees it up to date and still compiles nothing."""
    build, calls = fake_build
    holder = subprocess.Popen([sys.executable, "-c", "import fcntl, sys\n"
                               "lock = open(sys.argv[1], 'w'); fcntl.flock(lock, fcntl.LOCK_EX); print('locked', flush=True)\n"
                               "sys.stdin.readline()\n"
                               "open(sys.argv[2], 'w').write('x'); open(sys.argv[2] + '.srchash', 'w').write(sys.argv[3] + ' full\\n')\n",
                               build.LOCK, build.SAFE_LIB, build._src_hash()], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    try:
        assert holder.stdout.readline().strip() == "locked"
        waiter = threading.Thread(target=build.build_safe)
        waiter.start()
        time.sleep(0.5)
        assert waiter.is_alive() and calls == []
        holder.stdin.write("\n")
        holder.stdin.flush()
        waiter.join(timeout=30)
        assert not waiter.is_alive() and calls == [] and build.safe_lib_variants() == "full"
    finally:
        holder.kill()
        holder.wait()
