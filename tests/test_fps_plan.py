"""fps_plan (epnet_amd/csrc/fps_plan.h): which sampling kernel a call gets and what runs around it, as a pure function -- checked on
the host, without a GPU, by tests/fps_plan_selftest.cpp.

The pinned table was recorded from the dispatch code this plan replaced (fps_plain / fps_over_index and the five entry points
above them): that code was compiled for the host with its kernel launches recorded instead of issued, and every launch -- kernel
instantiation, grid, block, LDS bytes, arguments -- read back in the terms of a plan. `rows` prints one line per call of the
boundary table (22 cloud sizes x 9 sample counts x every pointer pattern of every entry point x two batch sizes, under the default
knobs and under each knob at one other value, plus the flawed calls and the limits on the batch); DIGESTS holds a SHA-256 prefix
of the old code's lines per (knobs, entry point), PICTURE a readable excerpt. Over the full sweep (every n up to 65537 x every legal
knob value) the old code and the plan disagreed on no call when this was recorded.

`sweep` walks that full sweep and asserts what used to live in comments: the index epilogue's preconditions, that prefix_out starts
at m only under a kernel that reports ties, that the stream and bigscene kernels never run without their running distances. It prints
every (family, waves, ppt) ever chosen: exactly what fps_run's ladders instantiate."""
import collections
import hashlib
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

ROWS = 128268
DIGESTS = {
    ("default", "fps"): "c90234c107002fdf",
    ("default", "fps_indexed"): "8ddcfa587dbfc0e6",
    ("default", "centres"): "e6ecaea69df0467d",
    ("default", "chain"): "723f970c118c7730",
    ("default", "chain_index"): "e01a4e0537ce6384",
    ("prune=0", "fps"): "ce970f401f285e6e",
    ("prune=0", "fps_indexed"): "c924c1cd477fddca",
    ("prune=0", "centres"): "0bf900a2024fb00f",
    ("prune=0", "chain"): "e90327152386a357",
    ("prune=0", "chain_index"): "3b4882a005c7d2f1",
    ("prune_min=4096", "fps"): "26fc6dfb0d789fe9",
    ("prune_min=4096", "fps_indexed"): "c107d02a7bdda520",
    ("prune_min=4096", "centres"): "ae203ea3c9f1a950",
    ("prune_min=4096", "chain"): "01d6f342d66e1054",
    ("prune_min=4096", "chain_index"): "5ac871fbf9a3e880",
    ("pwaves=8", "fps"): "99bbcb86becccf82",
    ("pwaves=8", "fps_indexed"): "f0b89e8b252b0083",
    ("pwaves=8", "centres"): "930b393ebb191286",
    ("pwaves=8", "chain"): "9d723d03d8c2808f",
    ("pwaves=8", "chain_index"): "514a1f7e4979c211",
    ("waves=4", "fps"): "f7ca15bfd8a99c57",
    ("waves=4", "fps_indexed"): "2c8a09dfe00b22a0",
    ("waves=4", "centres"): "903d6f7ea401e90c",
    ("waves=4", "chain"): "3164a2dff6d64cb0",
    ("waves=4", "chain_index"): "5afb2c0c40759ac0",
}

# epnet_sample_centres, two scenes, two samples, default knobs: n -> (without index and temp, with both)
PICTURE = {
    1: ("rc=-1", "stream<1,0>+gather"),
    63: ("rc=-1", "stream<1,0>+gather"),
    64: ("wave<1,1>", "wave<1,1>"),
    65: ("wave<1,2>", "wave<1,2>"),
    127: ("wave<1,2>", "wave<1,2>"),
    128: ("wave<1,2>", "wave<1,2>"),
    512: ("wave<1,8>", "wave<1,8>"),
    513: ("wave<8,2>", "wave<8,2>"),
    1023: ("wave<8,2>", "wave<8,2>"),
    1024: ("wave<8,2>", "wave<8,2>"),
    1025: ("pruned<4,8>+gather", "indexed<4,8>+gather"),
    2048: ("pruned<4,8>+gather", "indexed<4,8>+gather"),
    2049: ("pruned<4,16>+gather", "indexed<4,16>+gather"),
    4096: ("pruned<4,16>+gather", "indexed<4,16>+gather"),
    4097: ("pruned<4,32>+gather", "indexed<4,32>+gather"),
    8192: ("pruned<4,32>+gather", "indexed<4,32>+gather"),
    8193: ("pruned<8,32>+gather", "indexed<8,32>+gather"),
    16384: ("pruned<8,32>+gather", "indexed<8,32>+gather"),
    16385: ("rc=-1", "bigscene<16,0>+gather"),
    32768: ("rc=-1", "bigscene<16,0>+gather"),
    65536: ("rc=-1", "bigscene<16,0>+gather"),
    65537: ("rc=-1", "stream<16,0>+gather"),
}

# what fps_run instantiates: every one is chosen somewhere in the sweep, and nothing else ever is
LADDERS = ({"wave<%d,%d>" % (w, p) for w in (1, 2, 4, 8, 16) for p in (1, 2, 4, 8, 16)}
           | {"pruned<%d,%d>" % (w, p) for w in (4, 8) for p in (8, 16, 32)}
           | {"indexed<4,8>", "indexed<4,16>", "indexed<4,32>", "indexed<8,32>", "bigscene<16,0>", "stream<1,0>", "stream<16,0>"})


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path_factory.mktemp("fps_plan") / "fps_plan_selftest")
    # (a plain host build: the header must need nothing of HIP)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "epnet_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "fps_plan_selftest.cpp"), "-o", exe])
    return exe


def test_boundary_rows_equal_the_recorded_dispatch(selftest):
    out = subprocess.run([selftest, "rows"], capture_output=True, text=True, timeout=120)
    lines = out.stdout.splitlines(keepends=True)
    assert out.returncode == 0 and not [l for l in lines if l.startswith("FAILED")], out.stdout[-2000:]
    assert len(lines) == ROWS
    groups = collections.OrderedDict()
    for line in lines:
        t = line.split()
        groups.setdefault((t[0], t[1]), []).append(line)
    assert list(groups) == list(DIGESTS)
    for key, rows in groups.items():
        got = hashlib.sha256("".join(rows).encode()).hexdigest()[:16]
        assert got == DIGESTS[key], "the plan of %s / %s differs from the recorded dispatch; its rows begin\n%s" % (key + ("".join(rows[:20]),))
    follow = {"0": "", "1": "+gather", "2": "+index"}
    picture = {}
    for line in groups[("default", "centres")]:
        head, plan = line.split(" :", 1)
        h, p = head.split(), plan.split()
        if h[2] == "b=2" and h[4] == "m=2" and h[5] in ("p=0", "p=3") and h[6] == "f=0":
            picture.setdefault(int(h[3][2:]), {})[h[5]] = p[0] if len(p) == 1 else p[1] + follow[p[-1].split("=")[1]]
    assert {n: (d["p=0"], d["p=3"]) for n, d in picture.items()} == PICTURE


def test_full_sweep_holds_the_invariants_and_reaches_every_instantiation(selftest):
    slices = 8
    step = -(-65537 // slices)
    procs = [subprocess.Popen([selftest, "sweep", str(1 + i * step), str(min(65537, (i + 1) * step))], stdout=subprocess.PIPE, text=True)
             for i in range(slices)]
    chosen, plans = set(), 0
    for p in procs:
        out = p.communicate(timeout=1200)[0]
        assert p.returncode == 0 and "FAILED" not in out, out[-2000:]
        for line in out.splitlines():
            kind, value = line.split()
            if kind == "chosen":
                chosen.add(value)
            else:
                plans += int(value)
    print("%d plans; chosen: %s" % (plans, " ".join(sorted(chosen))))
    assert plans > 2 * 10 ** 9
    assert chosen == LADDERS
