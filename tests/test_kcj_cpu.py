"""CPU tests of the band Jacobian's K compaction rule (csrc/kcj_slots.h; mlp_kernel.h, KCJ): tests/kcj_host writes the
compacted operand, the k list and the padding lane by lane with the header's own arithmetic, walks the product loop's ring and compares the
compacted product with the full chain bit for bit, for every per-wave survivor count 0 ... 128 in each of the four waves' positions and 3000
random survivor words.  The rule is restated here from the survivor words alone: the k list is the survivors in the order in which the
full chain visits them (tile, component, lane group), padded with k = 0 to whole trips of four k tiles, at least one.  The program also runs
under ASan and UBSan (its arrays have exactly the kernel's sizes)."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program

SRC = "kcj_host/kcj_host.cpp"
HP, N_CASES = 512, 4 * 129 + 2 + 3000


def run(exe, tmp):
    dst = str(tmp / "kcj.bin")
    r = subprocess.run([exe, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(N_CASES), "bad", "0"]
    rec = np.fromfile(dst, np.int32).reshape(N_CASES, 18 + HP)
    return rec[:, :16].astype(np.uint32).reshape(-1, 4, 4), rec[:, 16], rec[:, 17], rec[:, 18:]


def expected_klist(w):
    """k list [k tile][lane group][component] of survivor words w[wave][lane group] (bit 4 f + i: feature 128 wave + 16 f + 4 g + i)."""
    chain = []
    for t in range(HP // 16):
        for s in range(4):
            for g in range(4):
                k = 16 * t + 4 * g + s
                if (int(w[k // 128][g]) >> (((k % 128) // 16) * 4 + s)) & 1:
                    chain.append(k)
    tot = len(chain)
    padded = max(64, (tot + 63) // 64 * 64)
    chain += [0] * (padded - tot)
    kl = np.full(HP, -1, np.int64)
    for pos, k in enumerate(chain):
        kl[((pos // 16) * 4 + pos % 4) * 4 + (pos % 16) // 4] = k * HP
    return tot, padded, kl


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kcj_host")
    return run(build_host_program(tmp, SRC, "kcj_host"), tmp)


def test_every_count_in_every_wave_position_is_covered(cases):
    words = cases[0]
    counts = np.array([[sum(bin(int(x)).count("1") for x in words[c, v]) for v in range(4)] for c in range(4 * 129)])
    for v in range(4):
        assert counts[v * 129:(v + 1) * 129, v].tolist() == list(range(129))
    assert cases[1][4 * 129] == 0 and cases[2][4 * 129] == 64 and cases[1][4 * 129 + 1] == 512      # no survivor: one trip of zeros


def test_k_list_is_the_full_chain_order_padded(cases):
    words, tot, padded, klist = cases
    for c in list(range(4 * 129 + 2)) + list(range(4 * 129 + 2, N_CASES, 7)):
        t, p, kl = expected_klist(words[c])
        assert (t, p) == (int(tot[c]), int(padded[c])), c
        live = kl >= 0
        assert np.array_equal(klist[c][live], kl[live]), c
    assert ((klist == -1) | ((klist >= 0) & (klist % HP == 0) & (klist // HP < HP))).all()


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = build_host_program(tmp_path, SRC, "kcj_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run(exe, tmp_path)
