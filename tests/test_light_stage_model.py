"""A numpy model of how the task kernels stage an Array or Run operand in the wave's LDS image (wave.hpp),
checked against plain set arithmetic:

  A. or_chunk_values: one single-bit OR (or XOR) per value of a lane's chunk of 8, slots past the chunk's
     live count sending 0 to whatever word their bits name (11 bits of word index: inside the image);
  B. toggles_fold_carry_lds + the PARITY probe of filter_rows_linear: the toggle image of a run list (bit start
     and bit end + 1 of every run) gets each 32-bit word's carry-in XORed into its bit 0, in the kernel's lane
     and row order (dword 4 * (64 k + L) + j of row k, lane L), and position y is a member iff
     popc(m << (~y & 31)) is odd for m = image[y >> 5].
"""
import numpy as np
import pytest

from light_stage_cases import run_lists, run_values

WORDS = 2048
M32 = 0xFFFFFFFF


def popc(x):
    x = np.asarray(x, np.uint64)
    n = np.zeros(x.shape, np.uint64)
    for s in range(0, 32):
        n += (x >> np.uint64(s)) & np.uint64(1)
    return n


def members(image):
    """The positions whose bit is set in a membership image."""
    bits = np.unpackbits(image.astype("<u4").view(np.uint8), bitorder="little")
    return np.nonzero(bits)[0].astype(np.uint32)


def stage_chunks(chunks, live, xor=False):
    """or_chunk_values over every chunk: chunks[c] = the 8 slot values of a lane, live[c] = its n."""
    image = np.zeros(WORDS, np.uint64)
    for x, n in zip(chunks, live):
        for i in range(8):
            wi = (int(x[i]) >> 5) & 2047
            bit = (1 << (int(x[i]) & 31)) if i < n else 0
            image[wi] = (int(image[wi]) ^ bit) if xor else (int(image[wi]) | bit)
    return image.astype(np.uint32)


def array_chunks(vals, pad):
    """A sorted value list as 16-byte chunks of 8 u16 slots; the last chunk's dead slots hold `pad`."""
    n = len(vals)
    nch = -(-n // 8)
    slots = np.full(nch * 8, pad, np.uint32)
    slots[:n] = vals
    return slots.reshape(nch, 8), [min(8, n - 8 * c) for c in range(nch)]


def run_chunks(runs):
    """stage_from_chunks' Run branch: 4 runs per lane chunk as (start, end + 1) slots, runs past the list read as
    zeros (the buffer load's range check), an end + 1 of 65536 dropped from the live count."""
    nr = len(runs)
    nch = -(-nr // 4)
    chunks, live = [], []
    for c in range(nch):
        x = []
        for k in range(4):
            s, e = runs[4 * c + k] if 4 * c + k < nr else (0, 0)  # a zero word: start 0, length - 1 = 0
            x += [s, e + 1]
        m = min(4, nr - 4 * c)
        n = 2 * m
        if x[2 * m - 1] >= 65536:
            n -= 1
        chunks.append(x)
        live.append(n)
    return chunks, live


def fold_carries(image):
    """toggles_fold_carry_lds, step by step as the wave does it."""
    t = image.astype(np.uint64).reshape(8, 64, 4)       # row k, lane L, dword j
    par = popc(t).sum(axis=2) & np.uint64(1)            # parity of the lane's 128-bit chunk per row
    incl = np.bitwise_xor.accumulate(par, axis=1)       # wave_xscan_xor over the lanes (each row's bit apart)
    excl = incl ^ par
    tot = incl[:, 63]
    rowc = np.concatenate([[0], np.bitwise_xor.accumulate(tot)[:-1]]).astype(np.uint64)  # parity of the rows below
    out = t.copy()
    c = rowc[:, None] ^ excl                             # carry into the lane's first dword
    for j in range(4):
        out[:, :, j] = t[:, :, j] ^ c
        c = popc(out[:, :, j]) & np.uint64(1)            # parity(t) ^ c: the carry into the next dword
    return out.reshape(WORDS).astype(np.uint32)


def probe(image, y):
    """filter_rows_linear<.., PARITY>: v_not, v_lshlrev (low 5 bits of the shift), v_bcnt, & 1."""
    y = np.asarray(y, np.uint64)
    m = image.astype(np.uint64)[(y >> np.uint64(5)).astype(np.int64)]
    sh = (~y) & np.uint64(31)
    return (popc((m << sh) & np.uint64(M32)) & np.uint64(1)).astype(bool)


# ------------------------------------------------------------------ A
ARRAYS = {
    "one": [40000], "seven": list(range(100, 107)), "eight": list(range(24, 32)), "nine": list(range(60, 69)),
    "one_word": list(range(64, 96)), "dense": list(range(0, 4096)), "edges": [31, 32, 63, 64, 65535],
}


@pytest.mark.parametrize("name", list(ARRAYS) + ["random511", "random512", "random513", "random4096"])
@pytest.mark.parametrize("xor", [False, True])
def test_single_bit_staging_of_an_array(name, xor):
    if name.startswith("random"):
        vals = np.sort(np.random.default_rng(3).choice(65536, int(name[6:]), replace=False))
    else:
        vals = np.array(ARRAYS[name])
    for pad in (0, 0xFFFF, int(vals[-1])):  # whatever the payload's last 16 bytes hold past the values
        chunks, live = array_chunks(vals, pad)
        assert np.array_equal(members(stage_chunks(chunks, live, xor)), vals.astype(np.uint32)), (name, pad)


@pytest.mark.parametrize("name,runs", run_lists(), ids=[n for n, _ in run_lists()])
@pytest.mark.parametrize("xor", [False, True])
def test_single_bit_staging_of_run_toggles(name, runs, xor):
    chunks, live = run_chunks(runs)
    want = sorted([s for s, _ in runs] + [e + 1 for _, e in runs if e + 1 < 65536])
    assert np.array_equal(members(stage_chunks(chunks, live, xor)), np.array(want, np.uint32))


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("name,runs", run_lists(), ids=[n for n, _ in run_lists()])
def test_carry_fold_and_parity_probe(name, runs):
    chunks, live = run_chunks(runs)
    folded = fold_carries(stage_chunks(chunks, live))
    want = np.zeros(65536, bool)
    want[run_values(runs)] = True
    got = probe(folded, np.arange(65536))
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])


def test_probe_of_a_membership_word_needs_the_top_bit_only():
    """The same shift on a membership image puts the value's own bit on top: the two probes differ only in
    what they count, which is why an image and its probe must be of one kind."""
    rng = np.random.default_rng(9)
    image = rng.integers(0, 1 << 32, WORDS, dtype=np.uint64).astype(np.uint32)
    y = np.arange(65536, dtype=np.uint64)
    m = image.astype(np.uint64)[(y >> np.uint64(5)).astype(np.int64)]
    top = ((m << ((~y) & np.uint64(31))) >> np.uint64(31)) & np.uint64(1)
    want = np.zeros(65536, bool)
    want[members(image)] = True
    assert np.array_equal(top.astype(bool), want)
