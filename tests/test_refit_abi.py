"""CPU test of the refit ABI (rt_refit_plan_bytes, rt_refit_plan_layout_get, rt_build_refit_plan, rt_refit): the header
declares the entry points, flags and layout, the Python names exist, the plan size follows its documented rule, and every
argument error is refused before any GPU work (the pointers below are never dereferenced: a correct library returns before it
touches them)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x100000         # a 256-byte aligned "device pointer" that must never be used
ENTRY_POINTS = ("rt_refit_plan_bytes", "rt_refit_plan_layout_get", "rt_build_refit_plan", "rt_refit")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)


def test_header_declares_the_refit_entry_points_flags_and_layout():
    src = _header()
    assert re.search(r"\bsize_t\s+rt_refit_plan_bytes\s*\(\s*uint32_t\s+\w+\s*\)", src)
    assert re.search(r"\bint\s+rt_refit_plan_layout_get\s*\(\s*uint32_t\s+\w+\s*,\s*rt_refit_plan_layout\s*\*", src)
    for fn in ("rt_build_refit_plan", "rt_refit"):
        assert re.search(r"\bint\s+" + fn + r"\s*\(\s*const\s+rt_build_input\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*uint32_t\s+\w+\s*,"
                         r"\s*void\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", src), fn
    for flag in ("RT_REFIT_BAD_TREE = 1", "RT_REFIT_PLAN_MISMATCH = 2", "RT_REFIT_PAIR_BROKEN = 4"):
        assert flag in src, flag
    m = re.search(r"typedef struct rt_refit_plan_layout \{(.*?)\} rt_refit_plan_layout;", src, flags=re.S)
    assert m and re.findall(r"size_t\s+(\w+);", m.group(1)) == ["status", "parents", "arrivals", "leaves", "total"]


def test_python_names(rt):
    for name in ENTRY_POINTS:
        assert name in rt.EXPORTS
        assert getattr(rt.lib(), name) is not None
    for name in ("RefitPlanBytes", "BuildRefitPlan", "Refit", "refit_status", "refit_plan_layout"):
        assert callable(getattr(rt, name)), name
    assert (rt.RT_REFIT_BAD_TREE, rt.RT_REFIT_PLAN_MISMATCH, rt.RT_REFIT_PAIR_BROKEN) == (1, 2, 4)
    assert "refit:" in rt.version()


def test_plan_bytes_rule(rt):
    up = lambda v: (v + 255) // 256 * 256
    for n in (0, 1, 2, 3, 1000, 4097, 1 << 20, 1_002_528, 10_000_000):
        S = rt.NodesBytes(n) // 32
        assert S == 4 * (n + 512)
        lay = rt.refit_plan_layout(n)
        assert rt.RefitPlanBytes(n) == lay.total == 256 + up(4 * S) + up(S) + up(4 * S), n
        assert lay.status == 0 and lay.parents == 256 and lay.arrivals == lay.parents + up(4 * S)
        assert lay.leaves == lay.arrivals + up(S) and lay.total == lay.leaves + up(4 * S)
        assert rt.RefitPlanBytes(n) <= 36 * n + 19 * 1024          # 36 bytes per triangle + a constant
        if n >= 4096:
            assert rt.RefitPlanBytes(n) <= 64 * n


def _inp(rt, n=100, tin=FAKE, tout=FAKE, nodes=FAKE):
    return ctypes.byref(rt._BuildInput(tin, tout, n, nodes, 0))


def test_argument_errors_before_gpu_work(rt):
    L = rt.lib()
    assert L.rt_refit_plan_layout_get(5, None) == -1
    for fn in (L.rt_build_refit_plan, L.rt_refit):
        assert fn(None, 0, 2, FAKE, None) == -1                               # no input
        assert fn(_inp(rt), 0, 2, None, None) == -1                           # no plan
        for odd in (FAKE + 4, FAKE + 64, FAKE + 128):
            assert fn(_inp(rt), 0, 2, odd, None) == -1                        # plan not 256-byte aligned
        for count in (8, 9, 0xFFFFFFFF):
            assert fn(_inp(rt), 0, count, FAKE, None) == -1                   # count > 7
        assert fn(_inp(rt, nodes=0), 0, 2, FAKE, None) == -1                  # no nodes
        assert fn(_inp(rt, tout=0), 0, 2, FAKE, None) == -1                   # no leaf records
        assert fn(_inp(rt, tout=FAKE + 16), 0, 2, FAKE, None) == -1           # records not 64-byte aligned
        assert fn(_inp(rt, nodes=FAKE + 32), 0, 2, FAKE, None) == -1          # nodes not 64-byte aligned
        assert fn(_inp(rt, tin=FAKE + 4), 0, 2, FAKE, None) == -1             # positions not 16-byte aligned
        assert fn(_inp(rt, n=(1 << 27) - 1023), 0, 2, FAKE, None) == -3       # n too large
        assert fn(_inp(rt, n=0xFFFFFFFF), 0, 2, FAKE, None) == -3
        # errors win over an empty input; n = 0 with valid arguments does nothing
        assert fn(_inp(rt, n=0), 0, 8, FAKE, None) == -1
        assert fn(_inp(rt, n=0), 0, 2, FAKE + 8, None) == -1
        assert fn(_inp(rt, n=0, tin=0, tout=0, nodes=0), 0, 2, FAKE, None) == 0
    assert L.rt_refit(_inp(rt, tin=0), 0, 2, FAKE, None) == -1                # refit needs the new positions
