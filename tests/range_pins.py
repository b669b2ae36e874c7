"""The reference's container-type assertions (`instanceof` pins) on Container.not / inot and on the RunContainers those
tests build, as data: the 30 lines tests/type_pins.py lists as "not on the path" of and/or/xor/andNot.  With
RoaringBitmap.add / remove / flip on the device they are on a path: a pin is (one container, op over [b, e) inside
its key, expected type), run on the restatement (test_range_ops_oracle.py) and through the device
(test_gpu_range_ops.py).  Paths are relative to /root/reference/RoaringBitmap/src/test/java/org/roaringbitmap/.

Inventory of the 30 lines:

  TestContainer.java (27)
    :255            inotTest10        Array.inot past every value                    -> Array
    :297            inotTest4         Array.inot, partial                            -> Array
    :318, :321      inotTest5         Bitmap.inot, partial, and back                 -> Bitmap, Bitmap
    :342, :345      inotTest6         Bitmap.inot inside one word, and back          -> Bitmap, Bitmap
    :365/367        inotTest7         Bitmap.inot down to 1773 values                -> Array   (if / else: 2 lines)
    :372/374        inotTest7 back    Array.inot up to 32763 values                  -> Bitmap  (if / else: 2 lines)
    :394, :398      inotTest8         Array.inot that contracts, and back            -> Array, Array
    :432            notTest10         Array.not past every value                     -> Array
    :457            notTest11         Array.not before every value                   -> Array
    :505            notTest4          Array.not, partial                             -> Array
    :526, :529      notTest5          Bitmap.not, partial, and back                  -> Bitmap, Bitmap
    :549, :552      notTest6          Bitmap.not inside one word, and back           -> Bitmap, Bitmap
    :572/574        notTest7          Bitmap.not down to 1773 values                 -> Array   (2 lines)
    :579/581        notTest7 back     Array.not up to 32763 values                   -> Bitmap  (2 lines)
    :601, :604      notTest8          Bitmap.not(4, 65536), and back                 -> Bitmap, Bitmap
    :624, :627      notTest9          Bitmap.not(0, 65201), and back                 -> Bitmap, Bitmap
  TestRunContainer.java (3)
    :1093           inot14once        a RunContainer filled by add(char) is still a RunContainer
    :2031           not14once         the same, before not
    :2058           not15             Run.not that keeps two long runs               -> Run

The "and back" steps take the first step's result as their input: its type is what the first pin asserts, its values
are computed here.  :1093 and :2031 assert the INPUT of a flip: `container.add((char) val)` num times on a
RunContainer (java.util.Random(1234), restated below) leaves a RunContainer of up to ~17000 runs, larger than the
Bitmap of the same set.  Restated as Run.add of the last value drawn onto the Run of the values before it, for the four
(num, rangeSize) shapes inot14 / not14 call (the line counts once); the flip that follows ((int) nextDouble() * ..
is 0: the range is [0, rangeSize)) is carried as a pin without an expected type, checked against the restatement.
Every input here is one a canonical RoaringBitmap can hold (Array <= 4096 < Bitmap, Runs sorted and non-adjacent), so
none needs the re-typing type_pins.py applies to its 32768-value ArrayContainers."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from type_pins import ARRAY, BITMAP, RUN, r, u

ADD, REMOVE, FLIP = 0, 1, 2


@dataclass
class RangePin:
    name: str
    cite: str                      # file:line of the assertion(s)
    input: Tuple[int, np.ndarray]  # (container type, low 16-bit values)
    op: int                        # ADD / REMOVE / FLIP
    rng: Tuple[int, int]           # [b, e) inside the container
    inplace: bool                  # inot / iadd (x.flip, x.add) or not / add (the static forms)
    expect: Optional[int]          # expected result container type (None: the reference does not pin it)
    card: Optional[int] = None     # expected result cardinality when the reference asserts it
    npins: int = 1                 # instanceof lines this case covers
    note: str = ""


def flipped(vals, b, e):
    x = np.zeros(65536, bool)
    x[np.asarray(vals, dtype=np.int64)] = True
    x[b:e] ^= True
    return np.nonzero(x)[0].astype(np.uint32)


class JavaRandom:
    """java.util.Random: the 48-bit LCG and nextDouble (26 + 27 bits)."""

    def __init__(self, seed: int):
        self.s = (seed ^ 0x5DEECE66D) & ((1 << 48) - 1)

    def _next(self, bits: int) -> int:
        self.s = (self.s * 0x5DEECE66D + 0xB) & ((1 << 48) - 1)
        return self.s >> (48 - bits)

    def next_double(self) -> float:
        return ((self._next(26) << 27) + self._next(27)) * (1.0 / (1 << 53))


def run14_values(num: int) -> List[int]:
    """The values inot14once / not14once add, in order (TestRunContainer.java:1080-1086, 2021-2026)."""
    g = JavaRandom(1234)
    return [int(g.next_double() * 65536) for _ in range(num)]


BIG = u([0, 2, 4, 6, 8], r(10, 32768))             # TestContainer's 32763-value content: a BitmapContainer
A5 = np.array([1, 3, 5, 7, 9], np.uint32)
A8 = u(r(0, 18), [21, 22, 23])
A40 = r(244, 284)


def _pair(name, cite1, cite2, t, vals, rng, inplace, e1, c1, e2, n1=1, n2=1):
    """A flip and the flip back: the second step's input is the first step's result, of the type the first pin
    asserts; the second result is the original content (checkContent)."""
    mid = flipped(vals, *rng)
    return [RangePin(name, cite1, (t, vals), FLIP, rng, inplace, e1, c1, npins=n1),
            RangePin(name + "/back", cite2, (e1, mid), FLIP, rng, inplace, e2, len(vals), npins=n2,
                     note="cardinality from checkContent(c, content)")]


PINS: List[RangePin] = [
    # ------------------------------------------------------------------ TestContainer.java, inot
    RangePin("TestContainer.inotTest10", "TestContainer.java:254-256", (ARRAY, [0, 2, 4]), FLIP, (65190, 65201), True,
             ARRAY, 14),
    RangePin("TestContainer.inotTest4", "TestContainer.java:296-298", (ARRAY, A5), FLIP, (4, 1000), True, ARRAY,
             999 - 4 + 1 - 3 + 2),
    *_pair("TestContainer.inotTest5", "TestContainer.java:317-319", "TestContainer.java:320-321", BITMAP, BIG,
           (4, 1000), True, BITMAP, 31773, BITMAP),
    *_pair("TestContainer.inotTest6", "TestContainer.java:341-343", "TestContainer.java:344-345", BITMAP, BIG,
           (4, 9), True, BITMAP, 32762, BITMAP),
    *_pair("TestContainer.inotTest7", "TestContainer.java:363-369", "TestContainer.java:370-375", BITMAP, BIG,
           (5, 31001), True, ARRAY, 1773, BITMAP, n1=2, n2=2),
    *_pair("TestContainer.inotTest8", "TestContainer.java:393-396", "TestContainer.java:397-398", ARRAY, A8,
           (5, 22), True, ARRAY, 10, ARRAY),
    # ------------------------------------------------------------------ TestContainer.java, not
    RangePin("TestContainer.notTest10", "TestContainer.java:431-433", (ARRAY, A40), FLIP, (51413, 51471), False,
             ARRAY, 40 + 58),
    RangePin("TestContainer.notTest11", "TestContainer.java:456-458", (ARRAY, A40), FLIP, (1, 59), False, ARRAY,
             40 + 58),
    RangePin("TestContainer.notTest4", "TestContainer.java:504-506", (ARRAY, A5), FLIP, (4, 1000), False, ARRAY,
             999 - 4 + 1 - 3 + 2),
    *_pair("TestContainer.notTest5", "TestContainer.java:525-527", "TestContainer.java:528-529", BITMAP, BIG,
           (4, 1000), False, BITMAP, 31773, BITMAP),
    *_pair("TestContainer.notTest6", "TestContainer.java:548-550", "TestContainer.java:551-552", BITMAP, BIG,
           (4, 9), False, BITMAP, 32762, BITMAP),
    *_pair("TestContainer.notTest7", "TestContainer.java:570-576", "TestContainer.java:577-582", BITMAP, BIG,
           (5, 31001), False, ARRAY, 1773, BITMAP, n1=2, n2=2),
    *_pair("TestContainer.notTest8", "TestContainer.java:600-602", "TestContainer.java:603-604", BITMAP, BIG,
           (4, 65536), False, BITMAP, 32773, BITMAP),
    *_pair("TestContainer.notTest9", "TestContainer.java:623-625", "TestContainer.java:626-627", BITMAP, BIG,
           (0, 65201), False, BITMAP, 32438, BITMAP),
    # ------------------------------------------------------------------ TestRunContainer.java
    RangePin("TestRunContainer.not15", "TestRunContainer.java:2044-2058", (RUN, u(r(0, 20000), r(40000, 60000))),
             FLIP, (15000, 25000), False, RUN),
]


def _run14(inplace: bool, cite: str):
    """:1093 / :2031 for the shapes of inot14 / not14, and the flips they go on to make."""
    out = []
    for i, (num, size) in enumerate([(10, 1), (10, 10), (1000, 100), (50000, 100)]):
        vals = run14_values(num)
        before, last = np.unique(np.asarray(vals[:-1], np.uint32)), vals[-1]
        tag = f"TestRunContainer.{'i' if inplace else ''}not14once({num},{size})"
        out.append(RangePin(tag + "/add", cite, (RUN, before), ADD, (last, last + 1), True, RUN,
                            npins=1 if i == 0 else 0,
                            note="container.add((char) val) keeps a RunContainer; one line, four shapes"))
        out.append(RangePin(tag + "/flip", cite, (RUN, np.unique(np.asarray(vals, np.uint32))), FLIP, (0, size),
                            inplace, None, npins=0, note="the flip itself: values checked, type not pinned"))
    return out


PINS += _run14(True, "TestRunContainer.java:1078-1095") + _run14(False, "TestRunContainer.java:2018-2033")


def n_pins() -> int:
    return sum(p.npins for p in PINS)
