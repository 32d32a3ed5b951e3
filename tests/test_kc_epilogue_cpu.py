"""CPU tests of the KC epilogue's slot arithmetic (csrc/kc_slots.h): tests/kc_epilogue_host emulates one workgroup's
epilogue lane by lane with the header's own arithmetic -- a survivor's rank from the wave's two survivor words, its slot, the k list,
the last wave's padding -- and must give exactly the operand image and k list the rule defines: the survivor at
chain position pos goes to slot (pos & ~7) | (pos & 1) * 4 | (pos & 7) >> 1 of its point, zeros pad up to the next multiple of 16, and
every dword of the live region is written exactly once (none outside it, no dword by two waves).  The rule is restated here in numpy."""
import subprocess

import numpy as np
import pytest

from tests._util import build_host_program

NW, HP, PT = 8, 512, 64
FULL = (1 << 64) - 1
EVEN = 0x5555555555555555           # chain positions 2 q: lane group 0
ODD = 0xAAAAAAAAAAAAAAAA            # lane group 1


def low(n):
    """the first n chain positions of a wave"""
    return (1 << n) - 1


def spread(n, rng):
    m = 0
    for c in rng.choice(64, n, replace=False):
        m |= 1 << int(c)
    return m


def structured():
    rng = np.random.default_rng(11)
    cases = {"all_zero": [0] * NW, "all_ones": [FULL] * NW, "only_g0": [EVEN] * NW, "only_g1": [ODD] * NW,
             "g0_then_g1": [EVEN, ODD] * 4, "one_wave_alive": [0, 0, 0, FULL, 0, 0, 0, 0], "last_wave_only": [0] * 7 + [low(5)]}
    for c in (0, 1, 31, 62, 63):
        cases["single_at_%d" % c] = [1 << c] * NW
    cases["single_mixed"] = [1 << ((9 * w + 4) % 64) for w in range(NW)]
    for n in (0, 1, 7, 8, 9, 63, 64):
        cases["count_%d_low" % n] = [low(n)] * NW
        cases["count_%d_spread" % n] = [spread(n, rng) for _ in range(NW)]
    # every residue of a wave's first position and of its count modulo 8: wave 0 sets the offset of wave 1, wave 1 has the count
    for a in range(8):
        for b in range(8):
            cases["off_%d_cnt_%d" % (a, b)] = [spread(a + 8 * ((a + b) % 3), rng), spread(b + 8 * (1 + (a * b) % 3), rng), spread((a + 3 * b) % 8, rng)] + [0] * 5
            cases["off_%d_cnt_%d_tail" % (a, b)] = [spread(a, rng), spread(b, rng)] + [spread(17, rng)] * 6
    for pad in range(16):             # totals with every padding
        n = (16 - pad) % 16 + 32
        cases["padding_%d" % pad] = [spread(n // 8 + (1 if w < n % 8 else 0), rng) for w in range(NW)]
        cases["padding_%d_short" % pad] = [0] * 6 + [spread((16 - pad) % 16, rng), 0]
    return cases


def random_sets(n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, NW), np.uint64)
    for i in range(n):
        dens = rng.choice([0.02, 0.1, 0.3, 0.47, 0.7, 0.95])
        bits = rng.random((NW, 64)) < dens * rng.random((NW, 1)) * 2
        out[i] = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    return out


def slot_of(pos):
    return (pos & ~7) | ((pos & 1) * 4) | ((pos & 7) >> 1)


def reference(cm, image=False):
    """tot, padded, k list and (optionally) the image [512 slots x 64 points as the operand's dwords] of one mask set"""
    klist = np.full(HP, -1, np.int32)
    img = np.full(HP * PT, -1.0, np.float32) if image else None
    pts = np.arange(PT)
    pos = 0
    for w in range(NW):
        for c in range(64):
            if (int(cm[w]) >> c) & 1:
                s = slot_of(pos)
                q, g = c >> 1, c & 1
                klist[s] = (w * 64 + (q >> 4) * 32 + ((q >> 2) & 3) * 8 + 4 * g + (q & 3)) * HP
                if image:
                    img[((s >> 2) * PT + pts) * 4 + (s & 3)] = ((w * 64 + c) * 64 + pts + 1).astype(np.float32)
                pos += 1
    tot, padded = pos, (pos + 15) // 16 * 16
    for pos in range(tot, padded):
        s = slot_of(pos)
        klist[s] = 0
        if image:
            img[((s >> 2) * PT + pts) * 4 + (s & 3)] = 0.0
    return tot, padded, klist, img


def run(exe, tmp, sets, dump):
    src, dst = str(tmp / "masks.bin"), str(tmp / "out.bin")
    np.ascontiguousarray(sets, np.uint64).tofile(src)
    r = subprocess.run([exe, src, dst] + (["dump"] if dump else []), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert r.stdout.split() == ["cases", str(len(sets)), "bad", "0"]
    rec = 3 + HP + (HP * PT if dump else 0)
    raw = np.fromfile(dst, np.int32).reshape(len(sets), rec)
    return raw


def check(raw, sets, dump):
    for rec, cm in zip(raw, sets):
        tot, padded, klist, img = reference(cm, dump)
        assert rec[0] == 1 and rec[1] == tot and rec[2] == padded
        assert (rec[3:3 + HP] == klist).all()
        if dump:
            assert rec[3 + HP:].view(np.float32).tobytes() == img.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    return build_host_program(tmp_path_factory.mktemp("kc_epilogue_host"), "kc_epilogue_host/kc_epilogue_host.cpp", "kc_epilogue_host")


def test_structured_mask_sets_cover_what_they_claim():
    cases = structured()
    offs, cnts, pads = set(), set(), set()
    for cm in cases.values():
        c = [bin(m).count("1") for m in cm]
        pads.add(-sum(c) % 16)
        for w in range(NW):
            if c[w]:
                offs.add((sum(c[:w]) % 8, c[w] % 8))
                cnts.add(c[w])
    assert offs == {(a, b) for a in range(8) for b in range(8)} and pads == set(range(16)) and {1, 7, 8, 9, 63, 64} <= cnts


def test_structured_mask_sets_image_and_k_list(host_program, tmp_path):
    sets = np.array(list(structured().values()), np.uint64)
    check(run(host_program, tmp_path, sets, True), sets, True)


def test_random_mask_sets(host_program, tmp_path):
    sets = random_sets(4000, 5)
    check(run(host_program, tmp_path, sets, False), sets, False)


def test_header_on_the_host_under_the_sanitizers(tmp_path):
    """exact-size arrays in the harness: a store outside the operand image or the k list is an error here"""
    exe = build_host_program(tmp_path, "kc_epilogue_host/kc_epilogue_host.cpp", "kc_epilogue_host_san",
                             ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    sets = np.concatenate([np.array(list(structured().values()), np.uint64), random_sets(300, 6)])
    check(run(exe, tmp_path, sets, False), sets, False)
