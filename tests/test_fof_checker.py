"""tests/fof_ref.py checked on the CPU: against a plain Python union-find on small clouds and a lattice full of ties, by-hand
cases (a pair at exactly r2 == B2, a NaN body), the sums against math.fsum, the worlds the device tests rely on, the host
model of the lock-free union (tools/fof_union_host.cpp) under ThreadSanitizer, and that the header, the ctypes mirror and
host/simulation.hpp declare the two calls.  No device."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fof_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["nbody_fof_labels", "nbody_fof_groups"]


def loop_labels(rec, b):
    """the header's words, one pair at a time, into a serial union-find; the label is the lowest index of the component"""
    x = [[float(c) for c in p] for p in rec["position"]]
    n = len(x)
    B2 = float(b) * float(b)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    for i in range(n):
        for j in range(i + 1, n):
            dx, dy, dz = x[j][0] - x[i][0], x[j][1] - x[i][1], x[j][2] - x[i][2]
            r2 = (dx * dx + dy * dy) + dz * dz
            if r2 < B2:
                a, c = find(i), find(j)
                parent[max(a, c)] = min(a, c)
    return np.array([find(i) for i in range(n)], np.int32)


def holed(rec):
    rec = rec.copy()
    rec["position"][2, 1] = np.nan
    return rec


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 40])
def test_the_restatement_is_the_union_find(nb, n, f64):
    import merge_ref
    worlds = [(merge_ref.cloud(nb, n, seed=n + 1, f64=f64, close=3), (1e-2, 1.0, 2.5, 100.0))]
    if n == 40:
        worlds += [(ref.lattice(nb, 3, f64), (0.5, 1.0, 1.001, 1.5, 10.0)), (holed(ref.lattice(nb, 3, f64)), (1.001, 1.5))]
    for rec, lengths in worlds:
        for b in lengths:
            lab = ref.labels(rec, b)
            want = loop_labels(rec, b)
            assert lab.dtype == np.int32 and np.array_equal(lab, want), b
            for min_members in (1, 2, 5):
                grp, mem = ref.groups(rec, b, min_members)
                sizes = {int(r): int((want == r).sum()) for r in set(want.tolist())}
                listed = sorted(r for r, c in sizes.items() if c >= min_members)
                assert grp["first"].tolist() == listed and grp["count"].tolist() == [sizes[r] for r in listed]
                assert grp["offset"].tolist() == np.concatenate([[0], np.cumsum(grp["count"])[:-1]]).astype(int).tolist()[:len(grp)]
                assert not grp["reserved"].any() and len(mem) == int(grp["count"].sum())
                for g in grp:
                    who = mem[g["offset"]:g["offset"] + g["count"]]
                    assert who[0] == g["first"] and (np.diff(who) > 0).all() and (want[who] == g["first"]).all()
                if min_members == 1:
                    assert sorted(mem.tolist()) == list(range(len(rec))), "every body exactly once"


def test_by_hand_cases(nb):
    two = np.zeros(2, nb.PARTICLE_DTYPE64)
    two["position"][1] = (3.0, 4.0, 0.0)
    two["velocity"][0], two["velocity"][1] = (1.0, 0.0, 0.0), (-1.0, 0.0, 2.0)
    two["mass"] = (1.0, 3.0)
    assert ref.labels(two, 5.0).tolist() == [0, 1], "r2 == B2 exactly: the comparison is strict"
    assert ref.labels(two, np.nextafter(5.0, 6.0)).tolist() == [0, 0]
    grp, mem = ref.groups(two, 6.0)
    assert len(grp) == 1 and mem.tolist() == [0, 1]
    g = grp[0]
    assert (g["first"], g["count"], g["offset"], g["reserved"], g["mass"]) == (0, 2, 0, 0, 4.0)
    assert g["mx"].tolist() == [9.0, 12.0, 0.0] and g["mv"].tolist() == [-2.0, 0.0, 6.0]
    assert len(ref.groups(two, 5.0)[0]) == 0 and len(ref.groups(two, 5.0, 1)[0]) == 2
    # bodies at 0, 1, 1.5, 2, 2.5 along x link through their neighbours; a NaN or infinite body is a group of its own
    line = np.zeros(5, nb.PARTICLE_DTYPE)
    line["position"][:, 0] = (0.0, 2.0, 1.0, 1.5, 2.5)
    line["mass"] = 1.0
    assert ref.labels(line, 1.25).tolist() == [0, 0, 0, 0, 0] and ref.labels(line, 0.75).tolist() == [0, 1, 1, 1, 1]
    assert ref.labels(line, 0.5).tolist() == [0, 1, 2, 3, 4], "0.5 apart exactly is not linked"
    for bad in (np.nan, np.inf):
        hole = line.copy()
        hole["position"][2, 1] = bad
        assert ref.labels(hole, 1.25).tolist() == [0, 1, 2, 1, 1]
    # the sums' order, written out again: 130 members -> lanes 0 and 1 hold three terms each
    t = np.array([1.0] + [2.0 ** -53] * 129)
    s = np.zeros(64)
    for k, v in enumerate(t):
        s[k % 64] += v
    for half in (32, 16, 8, 4, 2, 1):
        s[:half] += s[half:2 * half]
    assert ref.lane_tree_sum(t) == s[0] and ref.lane_tree_sum([]) == 0.0 and not np.signbit(ref.lane_tree_sum([]))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_sums_are_within_the_bound_of_fsum(nb, f64):
    """count - 1 additions at most touch a term: |sum - exact| <= n 2^-53 sum|term| with the products' own rounding inside
    the terms (they are the restatement's terms too)"""
    rec = ref.clumpy(nb, 1000, seed=1000, f64=f64)
    grp, mem = ref.groups(rec, ref.CLUMPY_B, 1)
    assert grp["count"].max() > 128
    x, v, m = (np.asarray(rec[f], np.float64) for f in ("position", "velocity", "mass"))
    for g in grp:
        who = mem[g["offset"]:g["offset"] + g["count"]]
        n = len(who)
        for got, terms in [(g["mass"], m[who])] + [(g["mx"][c], m[who] * x[who, c]) for c in range(3)] + \
                          [(g["mv"][c], m[who] * v[who, c]) for c in range(3)]:
            assert abs(got - math.fsum(terms)) <= n * 2.0 ** -53 * math.fsum(abs(terms))


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_the_worlds_of_the_device_tests(nb, f64):
    """what tests/test_fof_gpu.py relies on, checked on the reference itself"""
    rec = ref.clumpy(nb, 1000, seed=1000, f64=f64)
    lab = ref.labels(rec, ref.CLUMPY_B)
    roots, counts = np.unique(lab, return_counts=True)
    assert (counts >= 2).sum() >= 3 and (counts == 1).sum() >= 100 and (counts == 2).sum() >= 1
    tiles = [len(set((np.nonzero(lab == r)[0] // 256).tolist())) for r in roots]
    assert max(tiles) >= 3, "a group with members in three different 256-body tiles"
    assert (counts > 128).any() and ((counts > 64) & (counts <= 128)).any()
    b = 0.25
    rec, perm = ref.chain(nb, 1025, b, f64)
    assert (ref.labels(rec, b) == 0).all()
    rec, perm = ref.chain(nb, 1025, b, f64, cut=500)
    lab = ref.labels(rec, b)
    assert (lab[perm[:501]] == 0).all() and (lab[perm[501:]] == perm[501:].min()).all() and len(set(lab.tolist())) == 2
    assert (ref.labels(ref.star(nb, 600, b, f64), b) == 0).all()
    lab = ref.labels(ref.two_lattices(nb, 6, b, f64), b)
    assert (lab[0::2] == 0).all() and (lab[1::2] == 1).all()


def test_the_host_model_of_the_union_under_tsan(tmp_path):
    """tools/fof_union_host.cpp: csrc/fof_union.h against std::atomic<int> from 8 threads, built with -fsanitize=thread"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "fof_union_host")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-I", os.path.join(ROOT, "nbody-llm_amd", "csrc"),
                            os.path.join(ROOT, "tools", "fof_union_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr, run.stderr[-4000:]
    assert re.search(r"^fof_union_host ok: 2000 lists", run.stdout, flags=re.M), run.stdout


def test_header_and_mirrors_declare_the_calls(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text))
    mirror = open(os.path.join(ROOT, "nbody-llm_amd", "host", "simulation.hpp")).read()
    lib = C.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in nb.DECLARED_SYMBOLS and hasattr(lib, name)
        assert name + "(" in mirror, f"{name} is missing from host/simulation.hpp"
    assert "typedef struct NbodyGroup" in text
    assert [f for f, _ in nb.NbodyGroup._fields_] == list(ref.GROUP_DTYPE.names) == list(nb.GROUP_DTYPE.names)
    assert C.sizeof(nb.NbodyGroup) == nb.GROUP_DTYPE.itemsize == ref.GROUP_DTYPE.itemsize == 72
    assert nb.lib.nbody_abi_version() == 4
    assert nb.lib.nbody_fof_labels(None, 1.0, None, 0, None, None) == nb.NBODY_ERR_INVALID
    assert nb.lib.nbody_fof_groups(None, 1.0, 2, None, 0, None, None, 0, None) == nb.NBODY_ERR_INVALID


def test_the_header_states_the_rules():
    text = " ".join(open(os.path.join(ROOT, "include", "nbody_hip.h")).read().split())
    for words in ("THE LOWEST INDEX in i's connected component", "A GROUP OF ITS OWN", "sum[t] += sum[t + half] for half = 32, 16, ... 1",
                  "O(N^2 / 2) f64 pair terms", "a tree-accelerated neighbour search; periodic boundaries; linking in velocity space; unbinding"):
        assert words in text, words
