"""CPU tests of the ring of the compacted product loop (csrc/kc_slots.h, the sdfr_kc_ring_* rule; mlp_kernel.h, gemm_kc_body of the 64-row
kernels): tests/kc_ring_host walks the prologue and the loop with the header's own arithmetic for every even tile count from
2 to 64 and logs every k-list read, gather, operand read and chain step with the tile its emulated registers hold.  The rule is restated
here, from the log alone: every chain step (tile, component) happens exactly once and in order and reads its own tile's fragment and
operand; no index passes the last tile; no register is refilled before its chain step has read it; a gather is issued at least seven chain
steps before its use and addressed by the k-list words of its own tile, read at least one tile earlier; an operand is read one tile ahead.
The program also runs under ASan and UBSan (its arrays have exactly nkt tiles)."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program

SRC = "kc_ring_host/kc_ring_host.cpp"
COUNTS = list(range(2, 65, 2))
KLIST, GATHER, OPERAND, STEP = 0, 1, 2, 3
LEAD_STEPS = 7                                     # chain steps between a gather and the matrix instructions that read it


def run(exe, tmp):
    dst = str(tmp / "ring.bin")
    r = subprocess.run([exe, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(len(COUNTS)), "bad", "0"]
    rec = np.fromfile(dst, np.int32).reshape(-1, 6)
    assert sorted(set(rec[:, 0].tolist())) == COUNTS
    return {nkt: rec[rec[:, 0] == nkt][:, 1:] for nkt in COUNTS}


def check(nkt, ev):
    last = nkt - 1
    steps = [(int(e[4]), int(e[3])) for e in ev if e[0] == STEP]
    assert steps == [(t, c) for t in range(nkt) for c in range(4)]                  # every tile once, in order, component by component
    assert ((ev[:, 4] >= 0) & (ev[:, 4] <= last)).all()                             # no index beyond the last tile
    frag, words, oper = {}, {}, {}                 # (stage, component) -> [tile, clock, read]; stage -> [tile, clock]; stage -> [tile, clock, reads]
    for kind, clock, stage, comp, tile in ev.tolist():
        if kind == KLIST:
            words[stage] = [tile, clock]
        elif kind == GATHER:
            old = frag.get((stage, comp))
            assert old is None or old[2] == 1                                       # refilled only after exactly one chain step read it
            w = words[stage]
            assert w[0] == tile and w[1] <= clock - 1                               # addressed by its own tile's words, already read
            if clock >= 0:
                t = clock // 4
                assert comp == clock % 4 and stage == t % 2 and tile == min(t + 2, last)
                assert w[1] < 0 or w[1] <= clock - 4                                # (words read in the loop: a tile ahead of their gather)
            frag[(stage, comp)] = [tile, clock, 0]
        elif kind == OPERAND:
            old = oper.get(stage)
            assert old is None or old[2] == 4
            if clock < 0:
                assert tile == 0 and stage == 0
            else:
                assert clock % 4 == 0 and tile == min(clock // 4 + 1, last) and stage == (clock // 4 + 1) % 2      # one tile ahead
            oper[stage] = [tile, clock, 0]
        else:
            t = tile
            assert clock == 4 * t + comp and stage == t % 2
            f, o = frag[(stage, comp)], oper[stage]
            assert f[0] == t and f[2] == 0 and f[1] <= clock - LEAD_STEPS           # its own tile's fragment, gathered seven steps ahead
            assert o[0] == t and o[1] <= 4 * t - 4                                  # its own tile's operand, read one tile ahead
            f[2] += 1
            o[2] += 1


@pytest.fixture(scope="module")
def events(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kc_ring_host")
    return run(build_host_program(tmp, SRC, "kc_ring_host"), tmp)


@pytest.mark.parametrize("nkt", COUNTS)
def test_ring_rule(nkt, events):
    check(nkt, events[nkt])


def test_the_check_itself_sees_a_short_lead_and_a_wrong_tile(events):
    ev = events[6].copy()
    i = [k for k, e in enumerate(ev) if e[0] == GATHER and e[1] >= 0][0]
    check(6, ev)
    moved = np.concatenate([ev[:i], ev[i + 1:i + 30], ev[i:i + 1], ev[i + 30:]])     # the first loop gather issued 29 events later
    with pytest.raises(AssertionError):
        check(6, moved)
    wrong = ev.copy()
    j = [k for k, e in enumerate(ev) if e[0] == STEP and e[4] == 3][0]
    wrong[j, 4] = 2
    with pytest.raises(AssertionError):
        check(6, wrong)


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = build_host_program(tmp_path, SRC, "kc_ring_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for nkt, ev in run(exe, tmp_path).items():
        check(nkt, ev)
