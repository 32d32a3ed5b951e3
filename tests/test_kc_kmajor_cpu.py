"""CPU tests of the k-major image of the compacted operand (csrc/kc_slots.h, the sdfr_kcm_* functions): tests/kc_kmajor_host
emulates one workgroup's kc_store of the 64-row kernels lane by lane with the header's own arithmetic and must give exactly what the rule
defines -- the survivor at chain position pos owns row pos of the image (64 dwords), point p 32 + lp sits at dword 2 lp + p of its row, zero
rows pad up to the next multiple of 16, every dword of rows [0, padded) is written exactly once and none outside, the k list is the one of
the old image, and wave 0 pads.  The rule is restated here in numpy.  The mask sets are the ones of tests/test_kc_epilogue_cpu.py.

The bank check takes the byte addresses the header's functions give every lane -- for every survivor store and for every B read of the
product -- and applies the LDS service rules: an 8-byte store is served in groups of 16 consecutive lanes on 32 banks of 4 bytes, an 8-byte
read in groups of 32 lanes on 64 banks.  No group may have two lanes on one bank."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program
from tests.test_kc_epilogue_cpu import random_sets, slot_of, structured

NW, HP, PT = 8, 512, 64
SRC = "kc_kmajor_host/kc_kmajor_host.cpp"


def reference(cm, image=False):
    """tot, padded, k list and (optionally) the image [512 rows x 64 dwords] of one mask set"""
    klist = np.full(HP, -1, np.int32)
    img = np.full((HP, PT), -1.0, np.float32) if image else None
    pts = np.arange(PT)
    pos = 0
    for w in range(NW):
        for c in range(64):
            if (int(cm[w]) >> c) & 1:
                q, g = c >> 1, c & 1
                klist[slot_of(pos)] = (w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)) * HP
                if image:
                    img[pos, 2 * (pts % 32) + pts // 32] = ((w * 64 + c) * 64 + pts + 1).astype(np.float32)
                pos += 1
    tot, padded = pos, (pos + 15) // 16 * 16
    for pos in range(tot, padded):
        klist[slot_of(pos)] = 0
        if image:
            img[pos] = 0.0
    return tot, padded, klist, img


def run(exe, tmp, sets, mode=None):
    src, dst = str(tmp / "masks.bin"), str(tmp / "out.bin")
    np.ascontiguousarray(sets, np.uint64).tofile(src)
    r = subprocess.run([exe, src, dst] + ([mode] if mode else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(len(sets)), "bad", "0"]
    rec = 4 + HP + {None: 0, "dump": HP * PT, "addrs": NW * 32 * 64}[mode]
    return np.fromfile(dst, np.int32).reshape(len(sets), rec)


def check(raw, sets, dump):
    for rec, cm in zip(raw, sets):
        tot, padded, klist, img = reference(cm, dump)
        assert rec[0] == 1 and rec[1] == tot and rec[2] == padded
        assert rec[3] == (0 if padded > tot else -1)                     # the wave that padded
        assert (rec[4:4 + HP] == klist).all()
        if dump:
            assert rec[4 + HP:].view(np.float32).tobytes() == img.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("kc_kmajor_host"), SRC, "kc_kmajor_host")


def test_structured_mask_sets_image_and_k_list(host_program, tmp_path):
    sets = np.array(list(structured().values()), np.uint64)
    check(run(host_program, tmp_path, sets, "dump"), sets, True)


def test_random_mask_sets(host_program, tmp_path):
    sets = random_sets(4000, 5)
    check(run(host_program, tmp_path, sets), sets, False)


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    """exact-size arrays in the harness: a store outside the operand image or the k list is an error here"""
    exe = build_host_program(tmp_path, SRC, "kc_kmajor_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    sets = np.concatenate([np.array(list(structured().values()), np.uint64), random_sets(300, 6)])
    check(run(exe, tmp_path, sets), sets, False)


def conflicts(addr, group, banks):
    """addr [..., 64] byte addresses of 8-byte accesses (-1: lane inactive): the number of (group, bank) pairs that two lanes with different
    addresses hit.  A lane occupies the banks of both its dwords."""
    a = addr.reshape(-1, 64 // group, group).astype(np.int64)
    act = a >= 0
    bad = 0
    for d in (0, 4):
        bank = np.where(act, ((a + d) // 4) % banks, -1)
        s = np.sort(bank, axis=-1)
        bad += int(((s[..., 1:] == s[..., :-1]) & (s[..., 1:] >= 0)).sum())
    # (an 8-byte aligned lane's two dwords are an even bank and the next one: two lanes that share one share both, so counting per dword
    # misses nothing and identical addresses -- broadcasts -- do not occur among a store's lanes or a read's lanes here; checked below)
    s = np.sort(a, axis=-1)
    assert not ((s[..., 1:] == s[..., :-1]) & (s[..., 1:] >= 0)).any()
    return bad


def test_bank_rule_itself_sees_a_conflict():
    lanes = np.arange(64)
    assert conflicts(lanes * 8, 16, 32) == 0                             # 16 lanes on 32 consecutive dwords
    assert conflicts(lanes * 16, 16, 32) > 0                             # the old image's 16-byte stride: 8 banks for 32 lanes
    assert conflicts(lanes * 8, 32, 64) == 0
    assert conflicts(lanes * 256, 32, 64) > 0


def test_survivor_stores_are_conflict_free(host_program, tmp_path):
    sets = np.array(list(structured().values()), np.uint64)
    raw = run(host_program, tmp_path, sets, "addrs")
    addr = raw[:, 4 + HP:].reshape(len(sets), NW, 32, 64)
    alive = np.array([[[(int(cm[w]) >> (2 * q + g)) & 1 for g in range(2)] for q in range(32)] for cm in sets for w in range(NW)])
    assert ((addr.reshape(-1, 32, 2, 32) >= 0) == alive[..., None].astype(bool)).all()      # a lane group stores exactly its survivors
    assert (addr[addr >= 0] % 8 == 0).all()
    assert conflicts(addr, 16, 32) == 0


def test_product_reads_are_conflict_free(host_program, tmp_path):
    dst = str(tmp_path / "reads.bin")
    r = subprocess.run([host_program, "reads", dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    addr = np.fromfile(dst, np.int32).reshape(HP // 8, 4, 64)
    t, ks, lane = np.meshgrid(np.arange(HP // 8), np.arange(4), np.arange(64), indexing="ij")
    assert (addr == ((8 * t + 2 * ks + lane // 32) * 64 + 2 * (lane % 32)) * 4).all()      # row 8 t + 2 ks + lg, the lane's 8 bytes
    assert conflicts(addr, 32, 64) == 0
    # the two reads of one paired instruction (steps 0, 1 and 2, 3) are 512 bytes apart: its stride unit
    assert (addr[:, 1] - addr[:, 0] == 512).all() and (addr[:, 3] - addr[:, 2] == 512).all() and (addr[:, 2] - addr[:, 0] == 1024).all()
