"""CPU tests of the chain-order survivor words of the band Jacobian's compaction stage (csrc/kcjd_slots.h; mlp_kernel.h, KCJ):
tests/kcjd_host builds the chain words as the kernel's vote does, takes every lane's places with the header's masked population count and
checks them against the slot rule of csrc/kcj_slots.h.  The rule is restated here from the survivor words alone: the compacted chain is the
survivors in the order in which the full chain visits them (tile, component, lane group), and chain word j of a wave holds positions
32 j .. 32 j + 31 of that wave's 128.  Cases: 0, 1, 63, 64, 65, 128 and 512 survivors, an empty wave block, survivors only in the last lane
group of the last wave, densities 0.1, 0.5 and 0.9.  The program also runs under ASan and UBSan (its arrays have exactly the kernel's sizes)."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program

SRC = "kcjd_host/kcjd_host.cpp"
HP, N_CASES = 512, 2 + 5 * 20 + 40 + 12 + 600


def run(exe, tmp):
    dst = str(tmp / "kcjd.bin")
    r = subprocess.run([exe, dst], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(N_CASES), "bad", "0"]
    rec = np.fromfile(dst, np.int32).reshape(N_CASES, 34 + HP)
    return rec[:, :16].astype(np.uint32).reshape(-1, 4, 4), rec[:, 16:32].astype(np.uint32).reshape(-1, 4, 4), rec[:, 32], rec[:, 33], rec[:, 34:]


def expected_chain(w):
    """features in the order the full chain visits them, of survivor words w[wave][lane group] (bit 4 f + i: feature 128 wave + 16 f + 4 g + i)"""
    chain = []
    for t in range(HP // 16):
        for s in range(4):
            for g in range(4):
                k = 16 * t + 4 * g + s
                if (int(w[k // 128][g]) >> (((k % 128) // 16) * 4 + s)) & 1:
                    chain.append(k)
    return chain


def expected_words(w):
    """chain words of a wave from the visiting order alone: position c = 0 .. 127 of the wave is bit c % 32 of word c / 32"""
    out = np.zeros((4, 4), np.uint32)
    for wv in range(4):
        c = 0
        for t in range(8):
            for s in range(4):
                for g in range(4):
                    if (int(w[wv][g]) >> (4 * t + s)) & 1:
                        out[wv][c // 32] |= np.uint32(1 << (c % 32))
                    c += 1
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("kcjd_host")
    return run(build_host_program(tmp, SRC, "kcjd_host"), tmp)


def test_the_listed_cases_are_there(cases):
    words, _, tot, padded, _ = cases
    assert tot[0] == 0 and padded[0] == 64                              # no survivor: one trip of zeros
    for i, n in enumerate((1, 63, 64, 65, 128)):
        assert (tot[1 + 20 * i:21 + 20 * i] == n).all()
    assert tot[101] == 512 and padded[101] == 512
    for wv in range(4):
        assert not words[102 + 10 * wv:112 + 10 * wv, wv].any() and words[102 + 10 * wv:112 + 10 * wv].any()
    last = words[142:154]
    assert not last[:, :3].any() and not last[:, 3, :3].any() and last[:, 3, 3].all() and tot[142] == 32 and tot[143] == 1
    for i, d in enumerate((0.1, 0.5, 0.9)):
        assert abs(tot[154 + 200 * i:354 + 200 * i].mean() / 512 - d) < 0.02


def test_places_are_the_full_chain_order(cases):
    words, chain_words, tot, padded, feat = cases
    for c in range(N_CASES):
        chain = expected_chain(words[c])
        assert len(chain) == int(tot[c]) and int(padded[c]) == max(64, (len(chain) + 63) // 64 * 64), c
        assert feat[c][:len(chain)].tolist() == chain and (feat[c][len(chain):] == -1).all(), c
        assert np.array_equal(chain_words[c], expected_words(words[c])), c


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = build_host_program(tmp_path, SRC, "kcjd_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    run(exe, tmp_path)
