"""The eviction rule of the per-stream snapshot-panel pool (PerkScratch, csrc/fwx_perk.hip), as a pure function over
the entries' stamps and in-use marks: fwx_test_perk_scratch_victim.  An entry that a call still inside the library holds
is never the victim, whatever its stamp; the pool grows past its capacity for the moment instead.  CPU only; the pool
itself is exercised with more concurrent callers than it keeps by tests/test_gpu_threads.py.  Also the shape of the
pool hook fwx_test_pools, which needs no device either."""
import ctypes

from floydwarshall_amd import _lib


def victim(used, busy, cap):
    assert len(used) == len(busy)
    u = (ctypes.c_uint64 * max(len(used), 1))(*used)
    b = (ctypes.c_int * max(len(busy), 1))(*busy)
    return _lib.lib().fwx_test_perk_scratch_victim(u, b, len(used), cap)


def reference(used, busy, cap):
    """The rule restated: below capacity nothing goes; else the idle entry with the smallest stamp, if any."""
    if len(used) < cap:
        return -1
    idle = [i for i in range(len(used)) if not busy[i]]
    return min(idle, key=lambda i: used[i]) if idle else -1


def pools():
    out = (ctypes.c_uint64 * 12)()
    assert _lib.lib().fwx_test_pools(out, 0) == 3
    return [dict(zip(("capacity", "created", "destroyed", "peak"), (int(v) for v in out[4 * i:4 * i + 4])))
            for i in range(3)]


CAP = pools()[1]["capacity"]


def test_all_idle_gives_the_least_recently_used():
    used = [((7 * i) % CAP) + 10 for i in range(CAP)]         # a permutation when gcd(7, CAP) = 1
    assert len(set(used)) == CAP
    assert victim(used, [0] * CAP, CAP) == used.index(min(used))
    for at in (0, CAP // 2, CAP - 1):                         # the oldest first, in the middle, last
        stamps = [100 + i for i in range(CAP)]
        stamps[at] = 1
        assert victim(stamps, [0] * CAP, CAP) == at


def test_a_busy_lru_entry_is_passed_over_for_the_next_idle_one():
    used = list(range(1, CAP + 1))                            # entry 0 is the least recently used
    busy = [0] * CAP
    busy[0] = 1
    assert victim(used, busy, CAP) == 1
    busy[1] = 3                                               # (a count, not a flag: any non-zero mark is busy)
    assert victim(used, busy, CAP) == 2
    busy = [1] * CAP
    busy[CAP - 1] = 0                                         # only the MOST recently used entry is idle
    assert victim(used, busy, CAP) == CAP - 1


def test_all_busy_gives_none():
    assert victim(list(range(1, CAP + 1)), [1] * CAP, CAP) == -1
    assert victim(list(range(1, CAP + 5)), [1] * (CAP + 4), CAP) == -1


def test_below_capacity_gives_none():
    for count in (0, 1, CAP - 1):
        assert victim(list(range(1, count + 1)), [0] * count, CAP) == -1


def test_a_pool_grown_past_its_capacity_is_trimmed_from_its_idle_entries():
    """What a later `get` does after a burst: victims one after another until fewer than `cap` entries are kept."""
    used = [50, 3, 40, 9, 30, 1, 20, 7]
    busy = [0, 1, 0, 0, 0, 1, 0, 0]
    cap, gone = 5, []
    ids = list(range(len(used)))
    while True:
        v = victim(used, busy, cap)
        if v < 0:
            break
        gone.append(ids[v])
        del used[v], busy[v], ids[v]
    assert gone == [7, 3, 6, 4] and len(used) == cap - 1      # by stamp 7, 9, 20, 30; the busy 1 and 3 stay


def test_against_the_restated_rule_exhaustively_at_small_sizes():
    import itertools
    for count in range(0, 5):
        for perm in itertools.permutations(range(1, count + 1)):
            for marks in itertools.product((0, 1), repeat=count):
                for cap in range(0, 6):
                    assert victim(list(perm), list(marks), cap) == reference(perm, marks, cap), (perm, marks, cap)


def test_arguments_out_of_range():
    L = _lib.lib()
    one = (ctypes.c_uint64 * 1)(1)
    mark = (ctypes.c_int * 1)(0)
    assert L.fwx_test_perk_scratch_victim(one, mark, -1, 1) == -2
    assert L.fwx_test_perk_scratch_victim(one, mark, 1, -1) == -2
    assert L.fwx_test_perk_scratch_victim(None, mark, 1, 1) == -2
    assert L.fwx_test_perk_scratch_victim(one, None, 1, 1) == -2
    assert L.fwx_test_perk_scratch_victim(None, None, 0, 0) == -1     # an empty pool: nothing to evict


def test_pool_hook_reports_three_pools_without_a_device():
    ctx, perk, multi = pools()
    assert ctx["capacity"] >= 1 and perk["capacity"] >= 1 and multi["capacity"] >= 1
    for p in (ctx, perk, multi):
        assert p["destroyed"] <= p["created"] and p["peak"] <= p["created"]
    assert _lib.lib().fwx_test_pools(None, 0) == 3
