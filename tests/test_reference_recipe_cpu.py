"""The recipe that builds the reference's simple-knn and gridencoder into oracle/_ref (oracle/reference_build.py), checked
without a GPU.  With the reference tree at hand: what was copied differs from the originals only by the listed
substitutions, the protected kernel bodies are byte-identical, the manifest's hashes are those of the files, and every
binary exports its entry point.  Always: nothing under oracle/_ref and nothing that matches a reference source is in git.
"""
import hashlib
import json
import os
import subprocess

import pytest

from oracle import reference_build as RBuild

ROOT = RBuild.ROOT


def _reference_present():
    ref = RBuild.reference_dir()
    return all(os.path.isfile(os.path.join(ref, rel)) for rel in RBuild.SOURCES.values())


def _built():
    """The manifest of a build() that found the reference; a skip where there is no reference tree to compare with."""
    if not _reference_present():
        pytest.skip("no reference tree on this machine")
    assert os.path.exists(RBuild.MANIFEST), "oracle/_ref/MANIFEST.json missing: build() has not run"
    with open(RBuild.MANIFEST) as f:
        m = json.load(f)
    assert m.get("reference_missing") is False, "the reference tree is present and the manifest says it is missing"
    return m


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _git_files():
    try:
        out = subprocess.run(["git", "-C", ROOT, "ls-files", "-z"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        pytest.skip("not a git checkout")
    return [p for p in out.decode().split("\0") if p]


def test_substitutions_touch_only_what_they_may():
    for f, old, new, reason in RBuild.SUBSTITUTIONS:
        assert f in RBuild.SOURCES and reason.strip()
        launch = set(old) <= set("<> ") and set(new) <= set("<>")
        include = old.startswith("#include") and new.startswith("#include")
        api = old.startswith("cuda") and new.startswith("hip") and old.isidentifier() and new.isidentifier()
        assert launch or include or api, (f, old, new)


def test_function_spans_finds_definitions_not_calls():
    text = "int f(int a);\nint g() { return f(1); }\nint f(int a)\n{\n  // }\n  return '}' + a;\n}\nint h;\n"
    assert RBuild.function_spans(text, "f") == [(2, 6)]
    assert RBuild.function_spans(text, "g") == [(1, 1)]


def test_copies_differ_from_the_originals_only_by_the_listed_substitutions():
    m = _built()
    ref = RBuild.reference_dir()
    for name, rel in RBuild.SOURCES.items():
        orig = _read(os.path.join(ref, rel)).decode("utf-8").split("\n")
        copy = _read(os.path.join(RBuild.SRC_OUT, name)).decode("utf-8").split("\n")
        assert len(orig) == len(copy), name
        changed = [i for i, (a, b) in enumerate(zip(orig, copy)) if a != b]
        for i in changed:
            assert RBuild.apply_substitutions(name, orig[i]) == copy[i], (name, i + 1)
        if not any(f == name for f, *_ in RBuild.SUBSTITUTIONS):
            assert changed == [], name
        assert m["sources"][name]["from"] == rel


def test_protected_kernel_bodies_are_byte_identical():
    _built()
    ref = RBuild.reference_dir()
    for name, functions in RBuild.PROTECTED.items():
        orig = _read(os.path.join(ref, RBuild.SOURCES[name])).decode("utf-8")
        copy = _read(os.path.join(RBuild.SRC_OUT, name)).decode("utf-8")
        ol, cl = orig.split("\n"), copy.split("\n")
        for fn in functions:
            so, sc = RBuild.function_spans(orig, fn), RBuild.function_spans(copy, fn)
            assert so and so == sc, (name, fn)
            for a, b in so:
                assert b > a, (name, fn)                       # a body of several lines: a definition, not a stub
                assert ol[a:b + 1] == cl[a:b + 1], (name, fn)
    # the definitions found are the kernels meant: both coord2Morton (device function and kernel), one of each other
    knn = _read(os.path.join(RBuild.SRC_OUT, "simple_knn.cu")).decode("utf-8")
    assert len(RBuild.function_spans(knn, "coord2Morton")) == 2
    grid = _read(os.path.join(RBuild.SRC_OUT, "gridencoder.cu")).decode("utf-8")
    a, b = RBuild.function_spans(grid, "kernel_grid")[0]
    assert "wn_re" in "\n".join(grid.split("\n")[a:b + 1]) and b - a > 400


def test_manifest_hashes_match_the_files():
    m = _built()
    ref = RBuild.reference_dir()
    for name, rel in RBuild.SOURCES.items():
        assert m["sources"][name]["sha256_copied"] == hashlib.sha256(_read(os.path.join(RBuild.SRC_OUT, name))).hexdigest()
        assert m["sources"][name]["sha256_original"] == hashlib.sha256(_read(os.path.join(ref, rel))).hexdigest()
    assert sorted(m["builds"]) == ["grid_contract", "grid_strict", "knn_contract", "knn_strict"]
    for name, b in m["builds"].items():
        assert b["sha256"] == hashlib.sha256(_read(os.path.join(RBuild.OUT, b["path"]))).hexdigest(), name
        strict = "-ffp-contract=off" in b["flags"]
        assert strict == (b["variant"] == "strict") and not any(a.startswith("-ffp-contract") and a != "-ffp-contract=off"
                                                               for a in b["flags"]), name
        assert "--offload-arch=gfx950" in b["flags"]


def test_every_binary_exports_its_entry_point():
    m = _built()
    for name, b in m["builds"].items():
        path = os.path.join(RBuild.OUT, b["path"])
        syms = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, check=True).stdout.decode()
        if b["kind"] == "ctypes":
            for s in b["symbols"]:
                assert f" T {s}\n" in syms, (name, s)
        else:
            assert f" T PyInit_{b['module']}\n" in syms, name
            strings = _read(path)
            for s in b["symbols"]:
                assert s.encode() in strings, (name, s)


def test_nothing_under_oracle_ref_is_in_git():
    assert [p for p in _git_files() if p.startswith("oracle/_ref/") or p == "oracle/_ref"] == []
    ignored = subprocess.run(["git", "-C", ROOT, "check-ignore", "-q", "oracle/_ref/MANIFEST.json"]).returncode
    assert ignored == 0


def test_no_committed_file_matches_a_reference_source():
    """By content, whatever the name: against the copies in oracle/_ref/src (present after any build() that found the
    reference), the originals where the tree is at hand, and the hashes the manifest recorded."""
    files = _git_files()
    digests, texts = set(), []
    if os.path.exists(RBuild.MANIFEST):
        with open(RBuild.MANIFEST) as f:
            for s in json.load(f).get("sources", {}).values():
                digests |= {s["sha256_original"], s["sha256_copied"]}
    candidates = [os.path.join(RBuild.SRC_OUT, n) for n in RBuild.SOURCES]
    if _reference_present():
        candidates += [os.path.join(RBuild.reference_dir(), rel) for rel in RBuild.SOURCES.values()]
    for p in candidates:
        if os.path.isfile(p):
            data = _read(p)
            digests.add(hashlib.sha256(data).hexdigest())
            texts.append(data)
    if not digests and not texts:
        pytest.skip("nothing to compare with: no reference tree, no oracle/_ref/src, no hashes in a manifest")
    # distinctive lines of the sources (long, not a comment or a preprocessor line): none may appear in a committed file
    marks = set()
    for data in texts:
        for line in data.decode("utf-8", "replace").split("\n"):
            s = line.strip()
            if len(s) >= 60 and not s.startswith(("//", "/*", "*", "#")):
                marks.add(s.encode())
    for p in files:
        full = os.path.join(ROOT, p)
        if not os.path.isfile(full):
            continue
        data = _read(full)
        assert hashlib.sha256(data).hexdigest() not in digests, p
        if marks and len(data) <= 1 << 20:
            hit = marks & {line.strip() for line in data.split(b"\n")}
            assert not hit, (p, sorted(hit)[0][:80])


def test_without_a_reference_tree_the_recipe_succeeds_and_says_so(tmp_path):
    import sys
    empty, out = tmp_path / "no_reference", tmp_path / "out"
    empty.mkdir()
    env = dict(os.environ, **{RBuild.REFERENCE_ENV: str(empty)})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "reference_build.py"), "--out", str(out)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert len(p.stdout.strip().split("\n")) == 1 and "nothing built" in p.stdout
    with open(out / "MANIFEST.json") as f:
        m = json.load(f)
    assert m["reference_missing"] is True and m["builds"] == {}
    assert sorted(os.listdir(out)) == ["MANIFEST.json"]


def _run_recipe_without_reference(tmp_path, out):
    import sys
    empty = tmp_path / "no_reference"
    empty.mkdir(exist_ok=True)
    env = dict(os.environ, **{RBuild.REFERENCE_ENV: str(empty)})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "reference_build.py"), "--out", str(out)], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    assert len(p.stdout.strip().split("\n")) == 1
    with open(out / "MANIFEST.json") as f:
        return p.stdout, json.load(f)


def test_without_a_reference_tree_a_valid_carried_manifest_is_kept(tmp_path):
    """oracle/_ref built elsewhere and carried here: a build() without the reference tree leaves it alone, as long as every
    listed binary has its recorded hash; one binary changed or gone and the manifest says reference_missing."""
    out = tmp_path / "out"
    out.mkdir()
    blobs = {"liba.so": b"first binary", "modb.so": b"second binary"}
    for n, d in blobs.items():
        (out / n).write_bytes(d)
    carried = {"reference_missing": False, "sources": {}, "builds": {
        n: {"path": n, "sha256": hashlib.sha256(d).hexdigest(), "kind": "ctypes", "symbols": []} for n, d in blobs.items()}}
    text = json.dumps(carried, indent=1, sort_keys=True) + "\n"
    (out / "MANIFEST.json").write_text(text)
    said, m = _run_recipe_without_reference(tmp_path, out)
    assert "kept" in said and m == carried and (out / "MANIFEST.json").read_text() == text
    (out / "modb.so").write_bytes(b"not what was recorded")
    said, m = _run_recipe_without_reference(tmp_path, out)
    assert "nothing built, MANIFEST.json says so" in said and m["reference_missing"] is True and m["builds"] == {}
    # and a manifest that already says reference_missing stays one
    said, m = _run_recipe_without_reference(tmp_path, out)
    assert m["reference_missing"] is True
    (out / "MANIFEST.json").write_text(text)
    (out / "liba.so").unlink()
    said, m = _run_recipe_without_reference(tmp_path, out)
    assert m["reference_missing"] is True
