"""Recipe that builds two submodules of the reference itself into oracle/_ref/ (test infrastructure, never committed):

    submodules/simple-knn   -> libbsr_ref_knn_{strict,contract}.so            C entry point bsr_ref_knn (ref_wrap/knn_wrap.cpp)
    submodules/gridencoder  -> bsr_ref_gridencoder_{strict,contract}.so       the reference's own pybind module

The reference's sources are copied to oracle/_ref/src/ and reach the compiler unedited but for SUBSTITUTIONS below (every
one listed with its reason; tests/test_reference_recipe_cpu.py checks that the copies differ from the originals on those
lines only and that the PROTECTED kernel bodies are byte-identical).  Everything else CUDA-specific is answered by the
forwarding headers of oracle/ref_shim/ (ours: they forward to HIP, hipCUB and torch's ROCm headers by the names the reference
includes).  Each submodule is built twice:

    strict    -ffp-contract=off: every fp32 expression in source order.  What tests/knn_reference.py and
              tests/grid_reference.py claim to restate.
    contract  the compiler's default contraction: one legal "as nvcc would" build (nvcc contracts by default too), like
              libbsr_oracle_fma.so for the rasterizer.

The reference's rasterizer is NOT built: it needs the un-vendored GLM ("Oracle").

    python oracle/reference_build.py [--jobs N] [--out DIR]      N <= 8; DIR defaults to oracle/_ref

The reference tree is found through the environment variable BSR_REFERENCE_DIR (default: the directory `reference` next to
this repository).  Without it the recipe builds nothing: it keeps a manifest and binaries that were carried here from a
machine that has the tree, if every listed binary matches its recorded hash, and otherwise writes a manifest that says
"reference_missing": true.
oracle/_ref/MANIFEST.json lists what was built, the full command lines, and a hash of every source as copied; targets
whose inputs and command line have not changed are not rebuilt.
"""
from __future__ import annotations

import argparse
import concurrent.futures
import hashlib
import json
import os
import subprocess
import sys
import sysconfig
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(HERE, "_ref")
SRC_OUT = os.path.join(OUT, "src")
SHIM = os.path.join(HERE, "ref_shim")
WRAP = os.path.join(HERE, "ref_wrap")
MANIFEST = os.path.join(OUT, "MANIFEST.json")
REFERENCE_ENV = "BSR_REFERENCE_DIR"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
MAX_JOBS = 8

# copied name -> path inside the reference tree
SOURCES = {
    "simple_knn.cu": "submodules/simple-knn/simple_knn.cu",
    "simple_knn.h": "submodules/simple-knn/simple_knn.h",
    "gridencoder.cu": "submodules/gridencoder/src/gridencoder.cu",
    "gridencoder.h": "submodules/gridencoder/src/gridencoder.h",
    "bindings.cpp": "submodules/gridencoder/src/bindings.cpp",
}

# (file, old text, new text, reason) -- literal, applied to every line of the file.  Only include lines, launch-bracket
# spacing and runtime API names may appear here.
SUBSTITUTIONS = [
    ("simple_knn.cu", "<< <", "<<<", "launch-bracket spacing: clang does not join '<< <' into the launch token nvcc accepts"),
    ("simple_knn.cu", ">> >", ">>>", "launch-bracket spacing: the closing token of the same launches"),
]

# kernels and device functions whose bodies must reach the compiler byte-identical
PROTECTED = {
    "simple_knn.cu": ["coord2Morton", "boxMinMax", "boxMeanDist", "updateKBest", "distBoxPoint"],
    "gridencoder.cu": ["kernel_grid", "kernel_grid_backward", "kernel_input_backward", "get_grid_index", "fast_hash"],
}

COMMON = ["-O3", "-fPIC", "-shared", "-std=c++17", "-x", "hip", f"--offload-arch={ARCH}", "-w"]
VARIANT_FLAGS = {"strict": ["-ffp-contract=off"], "contract": []}   # contract: nothing, i.e. the compiler's default


def reference_dir() -> str:
    return os.environ.get(REFERENCE_ENV) or os.path.join(os.path.dirname(ROOT), "reference")


def apply_substitutions(name: str, text: str) -> str:
    for f, old, new, _ in SUBSTITUTIONS:
        if f == name:
            text = "\n".join(line.replace(old, new) for line in text.split("\n"))
    return text


def function_spans(text: str, name: str):
    """(first, last) 0-based line numbers of every definition `name(...) {...}` in text, template / attribute lines
    excluded: from the line holding the name to the line of the closing brace.  Brace matching skips comments, strings and
    character literals."""
    import re
    spans = []
    for m in re.finditer(r"\b" + re.escape(name) + r"\s*\(", text):
        i, depth = m.end(), 1
        while i < len(text) and depth:          # the parameter list
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        j = i
        while j < len(text) and text[j] in " \t\r\n":
            j += 1
        if text.startswith("const", j):
            j += 5
            while j < len(text) and text[j] in " \t\r\n":
                j += 1
        if j >= len(text) or text[j] != "{":
            continue                             # a call or a declaration, not a definition
        k, depth = j + 1, 1
        while k < len(text) and depth:
            two = text[k:k + 2]
            if two == "//":
                k = text.find("\n", k)
                k = len(text) if k < 0 else k
                continue
            if two == "/*":
                k = text.find("*/", k + 2)
                k = len(text) if k < 0 else k + 2
                continue
            if text[k] in "\"'":
                q = text[k]
                k += 1
                while k < len(text) and text[k] != q:
                    k += 2 if text[k] == "\\" else 1
                k += 1
                continue
            depth += {"{": 1, "}": -1}.get(text[k], 0)
            k += 1
        spans.append((text.count("\n", 0, m.start()), text.count("\n", 0, k - 1)))
    return spans


def _sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def _sha_file(path: str) -> str:
    with open(path, "rb") as f:
        return _sha(f.read())


def _tree_files(d: str):
    return sorted(os.path.join(r, f) for r, _, fs in os.walk(d) for f in fs)


def copy_sources(ref: str) -> dict:
    """Copy SOURCES with SUBSTITUTIONS applied -> {name: {"from", "sha256_original", "sha256_copied"}}.  A file whose
    content is already right is left alone (its time stamp too)."""
    os.makedirs(SRC_OUT, exist_ok=True)
    info = {}
    for name, rel in SOURCES.items():
        with open(os.path.join(ref, rel), "rb") as f:
            raw = f.read()
        new = apply_substitutions(name, raw.decode("utf-8")).encode("utf-8")
        dst = os.path.join(SRC_OUT, name)
        old = None
        if os.path.exists(dst):
            with open(dst, "rb") as f:
                old = f.read()
        if old != new:
            if os.path.exists(dst):
                os.chmod(dst, 0o644)
            with open(dst, "wb") as f:
                f.write(new)
        info[name] = {"from": rel, "sha256_original": _sha(raw), "sha256_copied": _sha(new)}
    return info


def _torch_paths():
    import torch
    from torch.utils import cpp_extension
    tdir = os.path.dirname(os.path.abspath(torch.__file__))
    inc = [p for p in cpp_extension.include_paths() if os.path.isdir(p)]
    return inc, os.path.join(tdir, "lib"), int(torch._C._GLIBCXX_USE_CXX11_ABI)


def targets() -> dict:
    """name -> {"output", "command", "inputs", "kind", "symbols"}"""
    t = {}
    t_inc, t_lib, abi = _torch_paths()
    for variant, vflags in VARIANT_FLAGS.items():
        out = f"libbsr_ref_knn_{variant}.so"
        t[f"knn_{variant}"] = {
            "kind": "ctypes", "output": out, "symbols": ["bsr_ref_knn"], "variant": variant,
            "inputs": [os.path.join(SRC_OUT, "simple_knn.cu"), os.path.join(SRC_OUT, "simple_knn.h"),
                       os.path.join(WRAP, "knn_wrap.cpp")],
            "command": [HIPCC] + COMMON + vflags + [f"-I{SHIM}", f"-I{SRC_OUT}", os.path.join(SRC_OUT, "simple_knn.cu"),
                                                    os.path.join(WRAP, "knn_wrap.cpp"), "-o", os.path.join(OUT, out)],
        }
        mod = f"bsr_ref_gridencoder_{variant}"
        # our own command line, not torch's extension builder: that one passes -D__HIP_NO_HALF_CONVERSIONS__ and
        # -D__HIP_NO_HALF_OPERATORS__, under which the reference's (__half) casts do not compile.
        # -Wno-c++11-narrowing: two of its launch sites narrow inside a dim3 initialiser, which nvcc lets pass.
        t[f"grid_{variant}"] = {
            "kind": "python", "output": mod + ".so", "module": mod, "variant": variant,
            "symbols": ["grid_encode_forward", "grid_encode_backward"],
            "inputs": [os.path.join(SRC_OUT, n) for n in ("gridencoder.cu", "gridencoder.h", "bindings.cpp")],
            "command": [HIPCC] + COMMON + vflags + [
                "-Wno-c++11-narrowing", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DHIPBLAS_V2",
                f"-D_GLIBCXX_USE_CXX11_ABI={abi}", f"-DTORCH_EXTENSION_NAME={mod}", "-DTORCH_API_INCLUDE_EXTENSION_H",
                f"-I{SHIM}", f"-I{SRC_OUT}"] + [f"-I{p}" for p in t_inc] + [f"-I{sysconfig.get_paths()['include']}"] + [
                os.path.join(SRC_OUT, "gridencoder.cu"), os.path.join(SRC_OUT, "bindings.cpp"),
                f"-L{t_lib}", "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip", "-ltorch", "-ltorch_python",
                "-o", os.path.join(OUT, mod + ".so")],
        }
    return t


def _toolchain() -> str:
    """The compiler's version line and, for the torch module, torch's version: part of every target's key, so that a ROCm or
    torch upgrade rebuilds (a module linked against another libtorch would not import)."""
    import torch
    v = subprocess.run([HIPCC, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    return v.strip().split("\n")[0] + " | torch " + torch.__version__


def _key(target: dict, toolchain: str) -> str:
    """Hash of everything a target's binary depends on: its command line, its inputs, the forwarding headers, the compiler
    and torch versions."""
    h = hashlib.sha256()
    h.update(toolchain.encode() + b"\0")
    h.update("\0".join(target["command"]).encode())
    for p in target["inputs"] + _tree_files(SHIM):
        h.update(p.encode() + b"\0" + _sha_file(p).encode())
    return h.hexdigest()


def _compile(name: str, target: dict):
    t0 = time.time()
    p = subprocess.run(target["command"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return name, p.returncode, p.stdout, time.time() - t0


def _write_manifest(m: dict):
    os.makedirs(OUT, exist_ok=True)
    tmp = MANIFEST + ".tmp"
    with open(tmp, "w") as f:
        json.dump(m, f, indent=1, sort_keys=True)
        f.write("\n")
    os.replace(tmp, MANIFEST)


def _rel(cmd):
    """Command line with this checkout's and the installation's directories shortened, for the manifest."""
    return [a.replace(ROOT, ".") for a in cmd]


def carried_builds():
    """Names of the builds of an existing manifest that says reference_missing: false, if there are any and EVERY binary it
    lists is there with the sha256 it recorded; else [].  oracle/_ref is built where the reference tree is and travels to
    machines where it is not: a build() there must not replace a valid manifest by one that says reference_missing."""
    try:
        with open(MANIFEST) as f:
            m = json.load(f)
        if m.get("reference_missing") is not False or not m.get("builds"):
            return []
        for b in m["builds"].values():
            if _sha_file(os.path.join(OUT, b["path"])) != b["sha256"]:
                return []
        return sorted(m["builds"])
    except (OSError, ValueError, KeyError, TypeError, AttributeError):
        return []


def main(argv=None) -> int:
    global OUT, SRC_OUT, MANIFEST
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jobs", type=int, default=MAX_JOBS)
    ap.add_argument("--out", default=OUT, help="output directory (default: oracle/_ref; tests point it elsewhere)")
    args = ap.parse_args(argv)
    OUT = os.path.abspath(args.out)
    SRC_OUT, MANIFEST = os.path.join(OUT, "src"), os.path.join(OUT, "MANIFEST.json")
    jobs = max(1, min(args.jobs, MAX_JOBS))
    ref = reference_dir()
    if not all(os.path.isfile(os.path.join(ref, rel)) for rel in SOURCES.values()):
        kept = carried_builds()
        if kept:
            print(f"oracle/_ref: no reference tree at {ref} (${REFERENCE_ENV}): nothing built; the {len(kept)} binaries "
                  f"carried here with their manifest match its hashes and are kept ({', '.join(kept)})")
            return 0
        _write_manifest({"reference_missing": True, "builds": {}, "sources": {}})
        print(f"oracle/_ref: no reference tree at {ref} (${REFERENCE_ENV}): nothing built, MANIFEST.json says so")
        return 0
    t_start = time.time()
    sources = copy_sources(ref)
    old = {}
    if os.path.exists(MANIFEST):
        try:
            with open(MANIFEST) as f:
                old = json.load(f).get("builds", {})
        except (ValueError, OSError):
            old = {}
    tg = targets()
    toolchain = _toolchain()
    keys = {n: _key(t, toolchain) for n, t in tg.items()}
    todo = [n for n, t in tg.items()
            if not (old.get(n, {}).get("key") == keys[n] and os.path.exists(os.path.join(OUT, t["output"])))]
    failed = {}
    seconds = {n: old.get(n, {}).get("compile_seconds") for n in tg}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        for name, rc, log, dt in ex.map(lambda n: _compile(n, tg[n]), todo):
            seconds[name] = round(dt, 1)
            if rc != 0:
                failed[name] = log
    builds = {}
    for n, t in tg.items():
        if n in failed:
            continue
        builds[n] = {"path": t["output"], "kind": t["kind"], "variant": t["variant"], "symbols": t["symbols"],
                     "module": t.get("module"), "flags": _rel(t["command"][1:]), "key": keys[n],
                     "sha256": _sha_file(os.path.join(OUT, t["output"])), "compile_seconds": seconds[n]}
    _write_manifest({"reference_missing": False, "arch": ARCH, "compiler": toolchain,
                     "substitutions": [list(s) for s in SUBSTITUTIONS], "sources": sources, "builds": builds})
    print(f"oracle/_ref: {len(todo)} of {len(tg)} reference binaries rebuilt in {time.time() - t_start:.0f} s "
          f"({', '.join(todo) if todo else 'all up to date'})")
    for n, log in failed.items():
        sys.stderr.write(f"oracle/_ref: building {n} FAILED:\n{log[-4000:]}\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
