"""CPU tests of the dense image of the 64-row kernels' compacted layers (csrc/kc_slots.h, the sdfr_kcd_* functions):
tests/kc_dense_host emulates one workgroup's kc_store lane by lane with the header's own arithmetic -- 32 unconditional 8-byte stores per
lane, feature j to row j, the k list at the places of the chain order, pad entries that name the zero row -- and then the product's reads
through that k list.  It must give exactly what the rule defines, restated here in numpy: the product visits exactly the survivors, in the
full chain's order, then pads that all read the zero row; every row of the image is written once and the zero row never; the k list has,
place by place, the features the parent's rule (sdfr_kc_slot, sdfr_kc_rank -- taken from tests/kc_kmajor_host, which runs them) enters.

The bank check takes the byte addresses of every store and read of the emulation and applies the LDS service rules with this file's own
copy: an 8-byte store is served in groups of 16 consecutive lanes on 32 banks of 4 bytes ((a / 4) % 32), an 8-byte read in the two halves
of the wave on 64 banks ((a / 4) % 64).  No group may have two lanes on one bank."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program
from tests.test_kc_epilogue_cpu import FULL, low, random_sets, slot_of, spread, structured

NW, HP, PT = 8, 512, 64
ROW_BYTES, ZERO_ROW = 256, 512
SRC = "kc_dense_host/kc_dense_host.cpp"


def chain_feature(w, c):
    q, g = c >> 1, c & 1
    return w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)


def required():
    """the cases the dense rule must be seen at, whatever the shared structured sets hold"""
    rng = np.random.default_rng(23)
    cases = {"no_survivor": [0] * NW, "all_512": [FULL] * NW,
             "single_feature_0": [1] + [0] * 7, "single_feature_511": [0] * 7 + [1 << 63]}
    assert chain_feature(0, 0) == 0 and chain_feature(7, 63) == 511
    for tot in (16, 32, 496, 1, 17, 497, 15, 31, 511):                    # totals = 0, 1, 15 (mod 16)
        per = [tot // 8 + (1 if w < tot % 8 else 0) for w in range(NW)]
        cases["total_%d_low" % tot] = [low(n) for n in per]
        cases["total_%d_spread" % tot] = [spread(n, rng) for n in per]
    return cases


def all_structured():
    cases = dict(structured())
    cases.update(required())
    return cases


def reference(cm):
    """tot, padded, the rows the chain visits [512] (-1 beyond padded), the k list [512] and the image [513 x 64] of one mask set"""
    visit = np.full(HP, -1, np.int32)
    klist = np.full(HP, -1, np.int32)
    img = np.zeros((HP + 1, PT), np.float32)
    pts = np.arange(PT)
    pos = 0
    for w in range(NW):
        for c in range(64):
            if (int(cm[w]) >> c) & 1:
                j = chain_feature(w, c)
                visit[pos] = j
                klist[slot_of(pos)] = j * ROW_BYTES
                img[j, 2 * (pts % 32) + pts // 32] = (j * 64 + pts + 1).astype(np.float32)
                pos += 1
    tot, padded = pos, (pos + 15) // 16 * 16
    for pos in range(tot, padded):
        visit[pos] = ZERO_ROW
        klist[slot_of(pos)] = ZERO_ROW * ROW_BYTES
    return tot, padded, visit, klist, img


N_STORE, N_READ = NW * 32 * 64, HP // 8 * 4 * 64


def run(exe, tmp, sets, mode=None):
    src, dst = str(tmp / "masks.bin"), str(tmp / "out.bin")
    np.ascontiguousarray(sets, np.uint64).tofile(src)
    r = subprocess.run([exe, src, dst] + ([mode] if mode else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(len(sets)), "bad", "0"]
    rec = 4 + 2 * HP + {None: 0, "dump": (HP + 1) * PT, "addrs": N_STORE + N_READ}[mode]
    return np.fromfile(dst, np.int32).reshape(len(sets), rec)


def check(raw, sets, dump):
    for rec, cm in zip(raw, sets):
        tot, padded, visit, klist, img = reference(cm)
        assert rec[0] == 1 and rec[1] == tot and rec[2] == padded
        assert rec[3] == (0 if padded > tot else -1)                     # the wave that entered the pads
        assert (rec[4:4 + HP] == klist).all()
        got = rec[4 + HP:4 + 2 * HP]
        assert (got == visit).all()                                      # exactly the survivors, in chain order, then pads on the zero row
        assert (got[tot:padded] == ZERO_ROW).all() and (got[:tot] < ZERO_ROW).all() and (got[padded:] == -1).all()
        if dump:
            assert rec[4 + 2 * HP:].view(np.float32).tobytes() == img.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("kc_dense_host"), SRC, "kc_dense_host")


@pytest.fixture(scope="module")
def parent_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("kc_kmajor_host_for_dense"), "kc_kmajor_host/kc_kmajor_host.cpp", "kc_kmajor_host")


def test_required_cases_are_what_they_claim():
    cases = required()
    tot = {k: sum(bin(m).count("1") for m in v) for k, v in cases.items()}
    assert tot["no_survivor"] == 0 and tot["all_512"] == 512 and tot["single_feature_0"] == 1 and tot["single_feature_511"] == 1
    assert {tot[k] % 16 for k in cases if k.startswith("total_")} == {0, 1, 15}
    for t in (16, 32, 496, 1, 17, 497, 15, 31, 511):
        assert tot["total_%d_low" % t] == t and tot["total_%d_spread" % t] == t


def test_structured_mask_sets_image_k_list_and_visits(host_program, tmp_path):
    sets = np.array(list(all_structured().values()), np.uint64)
    check(run(host_program, tmp_path, sets, "dump"), sets, True)


def test_random_mask_sets(host_program, tmp_path):
    sets = random_sets(1500, 7)
    check(run(host_program, tmp_path, sets), sets, False)


def test_k_list_is_the_parents_rule(host_program, parent_program, tmp_path):
    """place by place the feature that sdfr_kc_slot / sdfr_kc_rank enter in the k-major emulation (entry = feature x 512 there, pads 0)"""
    sets = np.concatenate([np.array(list(all_structured().values()), np.uint64), random_sets(500, 8)])
    dense = run(host_program, tmp_path, sets)
    src, dst = str(tmp_path / "pm.bin"), str(tmp_path / "po.bin")
    sets.tofile(src)
    r = subprocess.run([parent_program, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    parent = np.fromfile(dst, np.int32).reshape(len(sets), 4 + HP)
    for d, p in zip(dense, parent):
        tot, padded = int(p[1]), int(p[2])
        assert d[1] == tot and d[2] == padded and d[3] == p[3]
        surv = np.array([slot_of(pos) for pos in range(tot)], np.int64)
        pads = np.array([slot_of(pos) for pos in range(tot, padded)], np.int64)
        dk, pk = d[4:4 + HP], p[4:]
        assert (dk[surv] == pk[surv] // HP * ROW_BYTES).all() and (pk[surv] % HP == 0).all()
        assert (pk[pads] == 0).all() and (dk[pads] == ZERO_ROW * ROW_BYTES).all()
        rest = np.setdiff1d(np.arange(HP), np.concatenate([surv, pads]))
        assert (dk[rest] == -1).all() and (pk[rest] == -1).all()


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    """the stand-alone program with exact-size arrays: a store or read outside image + zero row or the k list is an error here"""
    exe = build_host_program(tmp_path, SRC, "kc_dense_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    sets = np.concatenate([np.array(list(all_structured().values()), np.uint64), random_sets(300, 9)])
    check(run(exe, tmp_path, sets), sets, False)


def conflicts(addr, group, banks):
    """addr [..., 64] byte addresses of 8-byte accesses (-1: lane inactive): the number of (group, bank) pairs that two lanes hit.  A lane
    occupies the banks of both its dwords; groups are `group` consecutive lanes."""
    a = addr.reshape(-1, 64 // group, group).astype(np.int64)
    act = a >= 0
    bad = 0
    for d in (0, 4):
        bank = np.where(act, ((a + d) // 4) % banks, -1)
        s = np.sort(bank, axis=-1)
        bad += int(((s[..., 1:] == s[..., :-1]) & (s[..., 1:] >= 0)).sum())
    return bad


def test_bank_rule_itself_sees_a_planted_conflict():
    lanes = np.arange(64)
    assert conflicts(lanes * 8, 16, 32) == 0                             # 16 lanes on 32 consecutive dwords
    assert conflicts(lanes * 16, 16, 32) > 0                             # a 16-byte stride: 8 banks for 16 lanes
    assert conflicts(lanes * 8, 32, 64) == 0                             # a half of the wave on one row of 256 bytes
    assert conflicts(lanes * 256, 32, 64) > 0                            # every lane on its own row: one bank
    planted = lanes * 8
    planted[5] = planted[3] + 128                                        # lane 5 on lane 3's banks, 32 dwords on
    assert conflicts(planted, 16, 32) > 0
    planted = lanes * 8
    planted[40] = planted[33] + 256
    assert conflicts(planted, 32, 64) > 0 and conflicts(np.where(lanes < 32, lanes * 8, -1), 32, 64) == 0


def test_stores_and_reads_are_conflict_free(host_program, tmp_path):
    sets = np.array(list(all_structured().values()), np.uint64)
    raw = run(host_program, tmp_path, sets, "addrs")
    store = raw[:, 4 + 2 * HP:4 + 2 * HP + N_STORE].reshape(len(sets), NW, 32, 64)
    read = raw[:, 4 + 2 * HP + N_STORE:].reshape(len(sets), HP // 8, 4, 64)
    # every lane stores every register, to the row of the register's feature: 64 rows of a wave, each written by one lane group
    w, q, lane = np.meshgrid(np.arange(NW), np.arange(32), np.arange(64), indexing="ij")
    feat = w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * (lane // 32) + (q & 3)
    assert (store == (feat * ROW_BYTES + 8 * (lane % 32))[None]).all()
    assert conflicts(store, 16, 32) == 0
    for rec, rd in zip(raw, read):
        nkt = int(rec[2]) // 8
        assert (rd[:nkt] >= 0).all() and (rd[nkt:] == -1).all()
        assert (rd[:nkt] % 8 == 0).all() and (rd[:nkt] < (HP + 1) * ROW_BYTES).all()
        # a half of the wave reads ONE row (its lane group's k word), the lane's 8 bytes of it
        rows = rd[:nkt].reshape(nkt, 4, 2, 32) // ROW_BYTES
        assert (rows == rows[..., :1]).all()
        assert (rd[:nkt].reshape(nkt, 4, 2, 32) % ROW_BYTES == 8 * np.arange(32)).all()
    assert conflicts(read[read[..., 0] >= 0], 32, 64) == 0
