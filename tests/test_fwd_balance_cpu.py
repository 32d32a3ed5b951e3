"""CPU tests of the grid forward's launch order from the last pass (csrc/tile_balance.h; include/sdfr.h: sdfr_mlp_forward_balanced;
DESIGN.md 3.1).  tests/fwd_balance_host walks the header's ranking as the device kernel does, on buffers of the state's exact sizes; the
result must be the rule restated here with numpy's stable sort: full chunks by (cost descending, static index ascending), a partial last
chunk in the last place, chunks whole -- for any cost words at all.  The CPU model of the tile schedule (tools/fwd_balance_model.py) is
recomputed and printed, with a loose guard.

Every vector runs at T = 1 ... 1000.  At T = 4096 (16 M comparisons a record) only 'ties', 'garbage' and 'equal' run, and under the
sanitizers only 'garbage': 'distinct', 'extremes' and the others are left out at that one size for run time."""
import ctypes
import subprocess

import numpy as np

from sdflabel_amd import _lib
from tests._util import build_host_program

SRC = "fwd_balance_host/fwd_balance_host.cpp"
# order_rows: T = 1, 2, 8, 11 + a partial chunk of 25 (the 9^3 grid), 27, 1000, 4096 chunks
ROWS = (64, 128, 512, 729, 1728, 64000, 4096 * 64)


def chunks(order_rows):
    return (order_rows + 63) // 64


def cost_vectors(T, rng):
    """all equal, all distinct, heavy ties, what a forward writes (multiples of 16 up to 7 x 512), garbage with negative and huge words"""
    i32 = np.iinfo(np.int32)
    out = {"zeros": np.zeros(T, np.int64), "equal": np.full(T, 1776, np.int64), "ascending": np.arange(T) * 16, "descending": -np.arange(T) * 16,
           "distinct": rng.permutation(T) * 16 + 1472, "two_values": rng.integers(0, 2, T) * 16 + 1600, "ties": rng.integers(92, 126, T) * 16,
           "garbage": rng.integers(i32.min, i32.max, T, endpoint=True), "extremes": rng.choice([i32.min, i32.min + 1, -1, 0, 1, i32.max - 1, i32.max], T)}
    return {k: v.astype(np.int32) for k, v in out.items()}


def fixed_order(order_rows, rng):
    D = round(order_rows ** (1.0 / 3.0))
    if D ** 3 == order_rows:                                    # the order the renderer uses
        out = np.empty(order_rows, np.int32)
        assert _lib.lib().sdfr_grid_tile_order(D, out.ctypes.data) == 0
        return out
    return rng.permutation(order_rows).astype(np.int32)


def reference(cost, fixed):
    """the rule: numpy's stable sort of the full chunks by descending cost (int64: -cost of the smallest int32 must not wrap)"""
    order_rows = fixed.shape[0]
    full = order_rows // 64
    rank_order = np.argsort(-cost[:full].astype(np.int64), kind="stable")
    return np.concatenate([fixed[c * 64:(c + 1) * 64] for c in rank_order] + [fixed[full * 64:]]).astype(np.int32)


def records():
    rng = np.random.default_rng(416)
    recs = []
    for order_rows in ROWS:
        fixed = fixed_order(order_rows, rng)
        for name, cost in cost_vectors(chunks(order_rows), rng).items():
            if order_rows == ROWS[-1] and name not in ("ties", "garbage", "equal"):      # 4096 chunks: 16 M comparisons a record
                continue
            recs.append((order_rows, name, cost, fixed))
    return recs


def run(exe, tmp, recs):
    src, dst = str(tmp / "in.bin"), str(tmp / "out.bin")
    np.concatenate([np.concatenate([np.array([n], np.int32), cost, fixed]) for n, _, cost, fixed in recs]).tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(len(recs)), "bad", "0"]
    return np.fromfile(dst, np.int32)


def check(out, recs):
    at = 0
    for order_rows, name, cost, fixed in recs:
        T, full = chunks(order_rows), order_rows // 64
        nxt, last, left, where = (out[at:at + order_rows], out[at + order_rows:at + order_rows + T], out[at + order_rows + T:at + order_rows + 2 * T],
                                  out[at + order_rows + 2 * T:at + order_rows + 3 * T])
        at += order_rows + 3 * T
        assert np.array_equal(nxt, reference(cost, fixed)), (order_rows, name)
        # a permutation of the static order with every chunk intact, the partial chunk last
        assert np.array_equal(np.sort(nxt), np.arange(order_rows)), (order_rows, name)
        heads = {int(fixed[c * 64]): c for c in range(full)}
        for p in range(full):
            c = heads[int(nxt[p * 64])]
            assert np.array_equal(nxt[p * 64:(p + 1) * 64], fixed[c * 64:(c + 1) * 64]) and where[p] == c, (order_rows, name, p)
        assert np.array_equal(nxt[full * 64:], fixed[full * 64:]) and (T == full or where[full] == full)
        assert np.array_equal(last, cost) and not left.any()
    assert at == out.shape[0]


def test_required_cases_are_there():
    recs = records()
    assert {chunks(n) for n, _, _, _ in recs} == {1, 2, 8, 12, 27, 1000, 4096} and 729 % 64 == 25
    by = {(n, k): c for n, k, c, _ in recs}
    assert len(np.unique(by[(64000, "distinct")])) == 1000 and len(np.unique(by[(64000, "equal")])) == 1
    assert len(np.unique(by[(64000, "ties")])) <= 34 and by[(64000, "garbage")].min() < -2 ** 30 and by[(64000, "garbage")].max() > 2 ** 30
    assert {-2 ** 31, 2 ** 31 - 1} <= set(by[(64000, "extremes")].tolist())


def test_next_order_is_the_stable_descending_sort(tmp_path):
    exe = build_host_program(tmp_path, SRC, "fwd_balance_host")
    recs = records()
    check(run(exe, tmp_path, recs), recs)


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    """the stand-alone program, buffers of the state's exact sizes: an index outside cost[], rank[], order[] or fixed[] is an error here"""
    exe = build_host_program(tmp_path, SRC, "fwd_balance_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    recs = [r for r in records() if r[0] != ROWS[-1] or r[1] == "garbage"]
    check(run(exe, tmp_path, recs), recs)


def test_state_size_and_argument_checks_need_no_device():
    """no decoder is dereferenced and no HIP call is made before the checks"""
    L = _lib.lib()
    assert L.sdfr_mlp_balance_bytes(64000) == 4 * (3 * 1000 + 4 + 2 * 64000) and L.sdfr_mlp_balance_bytes(729) == 4 * (3 * 12 + 4 + 2 * 729)
    assert L.sdfr_mlp_balance_bytes(0) == 0 and L.sdfr_mlp_balance_bytes(-3) == 0 and L.sdfr_mlp_balance_bytes(1 << 31) == 0
    fake = ctypes.create_string_buffer(64)
    p = ctypes.addressof(fake)
    for args, msg in [((None, p, 64, None), b"NULL"), ((p, None, 64, None), b"NULL"), ((p, p, 0, None), b"order_rows=0"),
                      ((p, p, 1 << 31, None), b"out of range")]:
        assert L.sdfr_mlp_balance_init(*args) == -1, args
        assert msg in L.sdfr_last_error(), (msg, L.sdfr_last_error())
    for args, msg in [((None, p, 64, p, None, p, 64, None), b"NULL"), ((p, None, 64, p, None, p, 64, None), b"NULL"),
                      ((p, p, 64, None, None, p, 64, None), b"NULL"), ((p, p, 64, p, None, None, 64, None), b"NULL"),
                      ((p, p, 64, p, None, p, 0, None), b"order_rows=0"), ((p, p, 64, p, None, p, -5, None), b"order_rows=-5"),
                      ((p, p, 100, p, None, p, 64, None), b"not a multiple"), ((p, p, -64, p, None, p, 64, None), b"out of range")]:
        assert L.sdfr_mlp_forward_balanced(*args) == -1, args
        assert msg in L.sdfr_last_error() and b"sdfr_mlp_forward_balanced" in L.sdfr_last_error(), (msg, L.sdfr_last_error())


def test_model_of_the_tile_schedule():
    """tools/fwd_balance_model.py on both fixtures, start latents 0, 1, 5, 17, 40 at D = 40.  When this test was written: tile cost 0.50 to
    0.66 M cycles, static order 5.7 to 6.4 % above the balanced sum / 256, heaviest first on the tile's own costs 2.5 to 3.1 %, on another
    start latent's costs 2.7 to 3.5 %, on the other fixture's 4.4 to 6.3 %.  The guard is loose: heaviest first is not worse than static."""
    from tools.fwd_balance_model import report
    rows = report(40)
    assert len(rows) == 10
    for name, start, res in rows:
        for g in (0, 1):                                         # CUs filled globally / per XCD
            assert res["lpt"][g] <= res["static"][g] + 1e-9, (name, start, res)
            assert res["lpt_other_crop"][g] <= res["static"][g] + 1e-9, (name, start, res)
            assert 0.0 <= res["lpt"][g] < 0.2
