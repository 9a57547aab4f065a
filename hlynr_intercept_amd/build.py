"""Builds the HIP shared library in-tree: hlynr_intercept_amd/libhlx.so (gfx950 only)."""
from __future__ import annotations

import fcntl
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB = os.environ.get("HLX_LIBRARY") or os.path.join(_HERE, "libhlx.so")   # HLX_LIBRARY: diagnostic builds
SAFE_LIB = os.path.join(_HERE, "libhlx_safe.so")
LOCK = os.path.join(_HERE, "libhlx.so.lock")     # held by every step of a build that writes: headers, libraries, sidecars
SOURCE = os.path.join(CSRC, "hlx_kernels.hip")
# not hlx_inst_gen.h: it decides in which translation unit an instantiation is compiled, not what the library contains
DEPS = ["hlx_kernels.hip", "hlx_host.inc", "hlx_obs.inc", "hlx_device.h", "hlx_kargs.h", "hlx_kcfg.h", "hlx_bake_gen.cpp", os.path.join("..", "..", "include", "hlx.h"),
        os.path.join("..", "..", "include", "hlx_obs.h"), "hlx_hrl.inc", os.path.join("..", "..", "include", "hlx_hrl.h"),
        "hlx_eval.inc", os.path.join("..", "..", "include", "hlx_eval.h")]

# Every compilation of hlx_kernels.hip -- product, safe, diagnostic and A/B builds -- starts from these flags and adds only defines
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-kernarg-preload-count=16",
         "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-Wno-unused-value"]
# -z defs: a launcher declared `extern template` in the host unit and defined in no part fails the link, not the dlopen
LINK = ["-shared", "-Wl,-z,defs"]
SAFE_FLAGS = ["-DHLX_HOT_FROM_MEMORY=1"]


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built (ROCm toolchain required)")


# Scenario presets whose constants are baked into dedicated step-kernel instantiations (literals instead of cross-lane
# fetches): (name, scenario, physics, overrides).  hlx_create uses a baked instantiation only when the configuration it
# is given derives exactly these constants; anything else runs the ordinary variants.
BAKED = [
    ("medium/base", "medium", "base", None),                      # BASELINE.json configs[1] (the headline)
    ("medium/v2dr", "medium", "v2dr", None),                      # configs[2]
    ("hard/config", "hard", "config", None),                      # configs[3]
    ("medium/config/volley3", "medium", "config", {"volley_mode": True, "volley_size": 3}),   # configs[4]
    ("medium/config", "medium", "config", None),                  # config.yaml as shipped
    ("medium/v2", "medium", "v2", None),                          # constructor defaults (train_flat_ppo.py)
    ("easy/config", "easy", "config", None),                      # configs[0]
]


def generate_baked(verbose: bool = False) -> str:
    """(Re)write csrc/hlx_baked_gen.h from the presets above with the g++-compiled generator (same build_kcfg as the
    library).  The file is committed; it is rewritten only when its content changes."""
    import ctypes as C
    import tempfile

    from . import _lib
    from .config import resolve_config
    from .scenarios import scenario_config

    out = os.path.join(CSRC, "hlx_baked_gen.h")
    gxx = shutil.which("g++") or shutil.which("c++")
    if not gxx:
        if os.path.exists(out):
            return out          # no host compiler: keep the committed tables (hlx_create verifies them anyway)
        raise RuntimeError("g++ not found and csrc/hlx_baked_gen.h is missing")
    with tempfile.TemporaryDirectory() as tmp:
        exe, rec = os.path.join(tmp, "bake_gen"), os.path.join(tmp, "cfgs.bin")
        subprocess.check_call([gxx, "-O1", "-std=c++17", "-o", exe, os.path.join(CSRC, "hlx_bake_gen.cpp"), "-lm"])
        with open(rec, "wb") as f:
            for name, scen, phys, over in BAKED:
                cfg = _lib.make_hlx_config(resolve_config(scenario_config(scen, phys, over)))
                f.write(name.encode().ljust(64, b"\0"))
                f.write(bytes(cfg))
        text = subprocess.check_output([exe, rec]).decode()
    old = open(out).read() if os.path.exists(out) else None
    if text != old:
        with open(out, "w") as f:
            f.write(text)
        if verbose:
            print("wrote", out)
    return out


def _src_hash() -> str:
    """sha256 over the contents of every source the library is built from (mtimes do not survive a copy to another box)."""
    import hashlib
    h = hashlib.sha256()
    for d in sorted(DEPS + ["hlx_baked_gen.h"]):
        path = os.path.join(CSRC, d)
        if os.path.exists(path):
            with open(path, "rb") as f:
                h.update(d.encode() + b"\0" + f.read())
    return h.hexdigest()


def needs_build() -> bool:
    """True when the library is missing or was built from different sources (content hash in libhlx.so.srchash)."""
    if os.environ.get("HLX_LIBRARY"):
        return False
    if not os.path.exists(LIB):
        return True
    try:
        with open(LIB + ".srchash") as f:
            return f.read().strip() != _src_hash()
    except OSError:
        mt = os.path.getmtime(LIB)          # a library without its sidecar: fall back to modification times
        return any(os.path.getmtime(os.path.join(CSRC, d)) > mt for d in DEPS)


INST_LIST = os.path.join(CSRC, "hlx_inst_gen.h")
PARTS = 8      # translation units the step kernel's instantiations are spread over (one hipcc each, run at once)
_INST_RE = __import__("re").compile(r"hlx_env_kernelILj(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELi(\d+)EE")


def instantiations(text: str):
    """The (SPEC, MODE, NOISE, PERSIST, LATE, BAKE) tuples of the step-kernel instantiations a disassembly listing names."""
    return sorted({tuple(int(x) for x in m.groups()) for m in _INST_RE.finditer(text)})


def write_inst_list(insts, verbose: bool = False) -> bool:
    """csrc/hlx_inst_gen.h: which instantiation is compiled in which part.  Heavy ones first, dealt round robin: a generic (run-time
    flags) or fused-rollout kernel takes several times as long to compile as a baked single-step one.  Committed, like
    hlx_baked_gen.h; rewritten only when its content changes.  Returns True if it was rewritten."""
    def weight(t):
        spec, mode, noise, persist, late, bake = t
        return -((4 if spec & 0x80000000 else 2 if not bake else 1) * (3 if persist else 2 if mode == 0 else 1) + (1 if noise else 0))
    order = sorted(insts, key=lambda t: (weight(t), t))
    lines = ["// generated by hlynr_intercept_amd/build.py from the instantiations of the last library it built: which translation-unit part",
             "// compiles which instantiation of the step kernel (hlx_kernels.hip, \"Launchers\").  A hint about WHERE to compile, never about what",
             "// exists: an instantiation that is not listed is compiled with the host code, as in a single translation unit."]
    for k in range(PARTS):
        lines.append(f"#if !defined(HLX_TU_PART) || HLX_TU_PART == {k}")
        for spec, mode, noise, persist, late, bake in order[k::PARTS]:
            lines.append(f"HLX_INST({spec}u, {mode}, {'true' if noise else 'false'}, {'true' if persist else 'false'}, {late}, {bake})")
        lines.append("#endif")
    text = "\n".join(lines) + "\n"
    old = open(INST_LIST).read() if os.path.exists(INST_LIST) else None
    if text == old:
        return False
    with open(INST_LIST, "w") as f:
        f.write(text)
    if verbose:
        print("wrote", INST_LIST, f"({len(order)} instantiations in {PARTS} parts)")
    return True


def _listed() -> int:
    try:
        return open(INST_LIST).read().count("HLX_INST(")
    except OSError:
        return 0


def _jobs() -> int:
    """Compilers at once: MAX_JOBS when set, never more than 16, nor more than this machine has CPUs."""
    return max(1, min(16, int(os.environ.get("MAX_JOBS") or 16), os.cpu_count() or 1))


def _compile(targets, verbose: bool = False) -> None:
    """hlx_kernels.hip once per (output, defines, split) target, all units in one pool.  split: PARTS + 1 units (hlx_kernels.hip,
    "Launchers") when csrc/hlx_inst_gen.h lists instantiations and HLX_SINGLE_TU is unset; a failure there: one unit."""
    import tempfile
    from concurrent.futures import ThreadPoolExecutor, wait

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=CSRC)

    def single(out, defines):
        return [_hipcc()] + FLAGS + defines + LINK + ["-o", out, SOURCE]

    split_ok = _listed() and not os.environ.get("HLX_SINGLE_TU")
    with tempfile.TemporaryDirectory(dir=_HERE) as tmp, ThreadPoolExecutor(_jobs()) as pool:
        work = []
        for i, (out, defines, split) in enumerate(targets):
            units = [["-DHLX_TU_HOST"]] + [[f"-DHLX_TU_PART={k}"] for k in range(PARTS)] if split and split_ok else []
            objs = [os.path.join(tmp, f"{i}.{k}.o") for k in range(len(units))]
            cmds = [[_hipcc()] + FLAGS + defines + u + ["-c", "-o", o, SOURCE] for u, o in zip(units, objs)] or [single(out, defines)]
            work.append((out, defines, objs, [pool.submit(run, c) for c in cmds]))
        for out, defines, objs, futures in work:
            wait(futures)           # every unit has ended before the fallback starts
            try:
                for f in futures:
                    f.result()
                if objs:
                    pool.submit(run, [_hipcc(), "--offload-arch=gfx950", "-fPIC"] + LINK + ["-o", out] + objs).result()
            except Exception as why:
                if not objs:
                    raise
                print(f"hlynr_intercept_amd.build: parallel build of {out} failed ({why}); compiling one translation unit", flush=True)
                pool.submit(run, single(out, defines)).result()


def safe_lib_variants() -> str:
    """'full', 'minimal' or '' for the libhlx_safe.so that is there."""
    try:
        with open(SAFE_LIB + ".srchash") as f:
            h, kind = f.read().split()
        return kind if h == _src_hash() and os.path.exists(SAFE_LIB) else ""
    except (OSError, ValueError):
        return ""


def _build(force: bool, verbose: bool, product: bool, safe: str) -> None:
    """libhlx.so if `product`, libhlx_safe.so if `safe` ('full', or 'minimal': the base kernel variant only), each if forced or out
    of date.  The product is renamed into place only after the hot-word check; both sidecars record the hash of what was compiled."""
    def todo():
        return product and (force or needs_build()), bool(safe) and (force or safe_lib_variants() not in ("full", safe))

    if not any(todo()):
        return
    with open(LOCK, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        do_lib, do_safe = todo()        # somebody else may have built it while this process waited
        if not (do_lib or do_safe):
            return
        generate_baked(verbose)
        src_hash = _src_hash()
        tmp, safe_tmp = f"{LIB}.{os.getpid()}.unverified", f"{SAFE_LIB}.{os.getpid()}.unverified"
        safe_only = bool(os.environ.get("HLX_SAFE_BUILD"))       # force the safe build (tests; a toolchain known to need it)
        targets = [(tmp, SAFE_FLAGS if safe_only else [], True)] if do_lib else []
        if do_safe:
            targets.append((safe_tmp, SAFE_FLAGS + (["-DHLX_AB_MINIMAL"] if safe == "minimal" else []), safe == "full"))
        _compile(targets, verbose)
        from . import hotcheck
        if do_lib and not safe_only:
            # the constants of the step kernel are fetched across lanes (v_readlane): a register-allocator spill of those two
            # VGPRs would silently corrupt them, so the code object is inspected before the library is put in place
            try:
                hotcheck.verify(tmp)
            except hotcheck.HotcheckToolsMissing:
                os.replace(tmp, LIB + ".unchecked")
                raise
            except hotcheck.HotcheckViolation as why:
                # This compiler does to a hot-word register what the cross-lane scheme cannot survive.  Not a reason to have no
                # library: the SAFE build reads the same constants from memory -- same results, slower (hlx_kernels.hip,
                # HLX_HOT_FROM_MEMORY) -- and says so (hlx_hot_words_from_memory(), bench.py's line, the marker file).
                os.replace(tmp, LIB + ".rejected")
                print(f"hlynr_intercept_amd.build: {why}\n  -> building the SAFE variant (-DHLX_HOT_FROM_MEMORY=1) instead", flush=True)
                safe_only = True
                _compile([(tmp, SAFE_FLAGS, True)], verbose)
            except Exception:
                os.replace(tmp, LIB + ".rejected")
                raise
        if do_lib:
            marker = LIB + ".safe"
            if safe_only:
                with open(marker, "w") as f:
                    f.write("built with -DHLX_HOT_FROM_MEMORY=1 (hot constants read from memory; see build.py)\n")
            elif os.path.exists(marker):
                os.remove(marker)
            os.replace(tmp, LIB)
        if do_safe:
            os.replace(safe_tmp, SAFE_LIB)
        for done, path, text in ((do_lib, LIB, src_hash), (do_safe, SAFE_LIB, f"{src_hash} {safe}")):
            if done:
                with open(path + ".srchash", "w") as f:
                    f.write(text + "\n")
        if do_lib:
            try:      # where the NEXT build compiles what: from what this one contains (a hint file: never a reason to fail)
                write_inst_list(instantiations(hotcheck.listing(LIB)), verbose)
            except Exception:
                pass


def build(force: bool = False, verbose: bool = False, with_safe: bool = False) -> str:
    """libhlx.so, built if forced or out of date (content hash in libhlx.so.srchash); `with_safe`: the full safe library too, its
    translation units in the same pool of compilers.  Returns the path of the product library."""
    _build(force, verbose, True, "full" if with_safe else "")
    return LIB


def build_safe(force: bool = False, minimal: bool = False) -> str:
    """The SAFE variant beside the product library (hlynr_intercept_amd/libhlx_safe.so, never loaded by default): what
    tests/test_safe_build_gpu.py compares with the product build bit for bit.  `minimal`: the base kernel variant only (seconds
    instead of minutes).  Returns the path; up to date when its sidecar holds the current source hash (+ the variant)."""
    _build(force, False, False, "minimal" if minimal else "full")
    return SAFE_LIB


def build_variant(out: str, defines) -> str:
    """hlx_kernels.hip with extra `defines` as one translation unit into `out`, under the build lock (A/B and diagnostic builds)."""
    with open(LOCK, "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        _compile([(out, list(defines), False)])
    return out


def build_stamps(level: int = 1) -> str:
    """Diagnostic build with s_memtime stamps (tools/diag_stamps.py); never used by the product path."""
    return build_variant(os.path.join(_HERE, "libhlx_stamps.so"), [f"-DHLX_STAMPS={level}"])


if __name__ == "__main__":
    print(build(force=True, verbose=True))
