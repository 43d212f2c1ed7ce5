"""RT_OPT_ROW_MIX's ordering policy on the host, through rt_order_units (the function the row
feedback calls on a cost snapshot): mode 0 is heaviest first, mode 1 the mixed order, which
must agree exactly with the restatement below.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from rtamd import capi

TAIL_PERMILLE = 20   # RT_ROW_MIX_TAIL_PERMILLE


def heaviest_first(umax):
    """Mode 0: by the unit's most expensive wave (clamped to 16 bits), ties to the lower unit."""
    k = np.minimum(np.asarray(umax, np.int64), 65535)
    return sorted(range(len(k)), key=lambda u: (-int(k[u]), u))


def classes(umax, usum):
    """(heavy, light) units in mode 0's order: work above the mean, plus the first unit."""
    s = heaviest_first(umax)
    n, total = len(s), int(np.asarray(usum, np.int64).sum())
    heavy = [u for k, u in enumerate(s) if int(usum[u]) * n > total or k == 0]
    light = [u for k, u in enumerate(s) if not (int(usum[u]) * n > total or k == 0)]
    return s, heavy, light, total


def split_tail(usum, light, total):
    """Light units merged / held back: the lightest one, then while <= TAIL_PERMILLE / 1000."""
    m = len(light) - 1
    tail = int(usum[light[m]])
    while m > 0 and (tail + int(usum[light[m - 1]])) * 1000 <= total * TAIL_PERMILLE:
        m -= 1
        tail += int(usum[light[m]])
    return light[:m], light[m:]


def mixed(umax, usum):
    """Mode 1, restated (exact integers)."""
    s, heavy, light, total = classes(umax, usum)
    n = len(s)
    if not any(int(usum[u]) * n > total for u in s) or not light:
        return s
    merged, tail = split_tail(usum, light, total)
    th = sum(int(usum[u]) for u in heavy)
    tl = sum(int(usum[u]) for u in merged)
    out, ch, cl, i, j = [], 0, 0, 0, len(merged)
    while i < len(heavy) or j > 0:
        if i < len(heavy) and (j == 0 or cl * th >= ch * tl):
            ch += int(usum[heavy[i]])
            out.append(heavy[i])
            i += 1
        else:
            j -= 1
            cl += int(usum[merged[j]])
            out.append(merged[j])
    return out + tail


def c2_like(n, seed):
    """40 % of the units at 30 k-60 k, 60 % at 3 k-6 k (a unit = 30 waves: sum ~ 20 maxima)."""
    rng = np.random.default_rng(seed)
    heavy = rng.random(n) < 0.4
    umax = np.where(heavy, rng.integers(30000, 60001, n), rng.integers(3000, 6001, n)).astype(np.uint32)
    usum = (umax.astype(np.uint64) * rng.integers(12, 29, n)).astype(np.uint32)
    return umax, usum


def cases():
    big = capi.ROW_PERM_MAX
    out = {"c2_like_1080": c2_like(1080, 1), "c2_like_135": c2_like(135, 2), "c2_like_max": c2_like(big, 3)}
    out["all_equal"] = (np.full(96, 4000, np.uint32), np.full(96, 90000, np.uint32))
    mx, sm = np.full(64, 3500, np.uint32), np.full(64, 70000, np.uint32)
    mx[17], sm[17] = 52000, 1300000
    out["one_heavy"] = (mx, sm)
    out["all_saturated"] = (np.full(200, 65535, np.uint32), np.full(200, 65535 * 30, np.uint32))
    out["n1"] = (np.array([700], np.uint32), np.array([9000], np.uint32))
    out["n2"] = (np.array([700, 41000], np.uint32), np.array([9000, 600000], np.uint32))
    rng = np.random.default_rng(7)   # the heaviest wave sits in a unit of little work
    mx, sm = c2_like(300, 8)
    mx[5], sm[5] = 65000, 66000
    out["heaviest_wave_in_light_unit"] = (mx, sm)
    out["random_uncorrelated"] = (rng.integers(0, 70000, 777).astype(np.uint32),
                                  rng.integers(0, 2**32, 777, dtype=np.uint64).astype(np.uint32))
    return out


CASES = cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_mode0_is_heaviest_first_ties_to_the_lower_unit(name):
    umax, usum = CASES[name]
    assert capi.order_units(umax, usum, 0).tolist() == heaviest_first(umax)


def test_mode0_random_and_saturated_costs():
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 64, 1080, capi.ROW_PERM_MAX):
        umax = rng.integers(0, 65536, n).astype(np.uint32)
        umax[rng.random(n) < 0.3] = 65535          # saturated waves: many ties
        umax[rng.random(n) < 0.1] = 70000          # above 16 bits: clamped, ties with 65535
        usum = rng.integers(0, 2**31, n).astype(np.uint32)
        assert capi.order_units(umax, usum, 0).tolist() == heaviest_first(umax), n


@pytest.mark.parametrize("name", sorted(CASES))
def test_mode1_agrees_with_the_restatement_and_its_properties(name):
    umax, usum = CASES[name]
    n = len(umax)
    got = capi.order_units(umax, usum, 1).tolist()
    assert sorted(got) == list(range(n))                          # a permutation
    assert got == capi.order_units(umax, usum, 1).tolist()        # deterministic
    s, heavy, light, total = classes(umax, usum)
    assert got[0] == s[0]                                         # the largest maximum first
    assert [u for u in got if u in set(heavy)] == heavy           # heavy: mode 0's relative order
    assert got == mixed(umax, usum)
    if any(int(usum[u]) * n > total for u in s) and light:
        merged, tail = split_tail(usum, light, total)
        assert len(tail) >= 1 and got[n - len(tail):] == tail     # the final stretch is light
        # balance: while heavy units remain, |cl / TL - ch / TH| stays within one largest
        # unit's work (the greedy step overshoots by at most the unit it just placed)
        th, tl = sum(int(usum[u]) for u in heavy), sum(int(usum[u]) for u in merged)
        wmax = int(np.asarray(usum, np.int64).max())
        hs, ch, cl, left = set(heavy), 0, 0, len(heavy)
        for u in got[:n - len(tail)]:
            if u in hs:
                ch += int(usum[u])
                left -= 1
            else:
                cl += int(usum[u])
            if left == 0:
                break
            assert abs(cl * th - ch * tl) <= wmax * max(th, tl), (name, u)


def test_all_equal_is_identity():
    umax, usum = CASES["all_equal"]
    assert capi.order_units(umax, usum, 1).tolist() == list(range(len(umax)))
    umax, usum = CASES["all_saturated"]
    assert capi.order_units(umax, usum, 1).tolist() == list(range(len(umax)))


def test_c2_like_mix_interleaves_the_classes():
    """Every tenth of the merged stretch holds units of both classes."""
    umax, usum = CASES["c2_like_1080"]
    got = capi.order_units(umax, usum, 1).tolist()
    s, heavy, light, total = classes(umax, usum)
    merged, tail = split_tail(usum, light, total)
    hs = set(heavy)
    body = got[:len(got) - len(tail)]
    for k in range(10):
        part = body[k * len(body) // 10:(k + 1) * len(body) // 10]
        assert any(u in hs for u in part) and any(u not in hs for u in part), k


def test_bad_arguments():
    lib = capi.load()
    mx = (C.c_uint32 * 4)(1, 2, 3, 4)
    perm = (C.c_int16 * 4)()
    bad = capi.RT_ERR_INVALID_ARG
    assert lib.rt_order_units(mx, mx, -1, 0, perm) == bad
    assert lib.rt_order_units(mx, mx, capi.ROW_PERM_MAX + 1, 0, perm) == bad
    assert lib.rt_order_units(None, mx, 4, 0, perm) == bad
    assert lib.rt_order_units(mx, None, 4, 1, perm) == bad
    assert lib.rt_order_units(mx, mx, 4, 1, None) == bad
    assert lib.rt_order_units(mx, mx, 4, 2, perm) == bad
    assert lib.rt_order_units(mx, mx, 4, 1, perm) == capi.RT_OK
    assert lib.rt_order_units(mx, mx, 0, 1, perm) == capi.RT_OK
