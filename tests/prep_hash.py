"""Python mirror of the tag hash of vartrix_amd/csrc/vtx_prep_core.h (vtx_hash_bytes) and of the barcode table (table_build /
table_probe), and what follows from the hash's shape: every step ``h ^= w; h *= p; h ^= h >> 29`` is a bijection of the 64-bit state,
so for any string, any other choice of its earlier words and any seed there is exactly ONE last word that gives the same 64-bit hash.
The constructors below compute it.  tests/test_prep_core.py proves the mirror against the core and every constructed pair against
both; tests/prep_cases.py builds its colliding barcodes and UMIs with them."""
M = (1 << 64) - 1
FNV0 = 0xcbf29ce484222325
PRIME = 0x100000001b3
UMI_SEED0 = 0x9e3779b97f4a7c15          # raw_prepare's first UMI seed; the barcode table hashes with seed 0
TABLE_MIN_SLOTS = 16


def next_seed(seed: int) -> int:
    return (seed * 0xd1342543de82ef95 + 1) & M


def _step(h: int, w: int) -> int:
    h ^= w
    h = (h * PRIME) & M
    return h ^ (h >> 29)


def _words(p: bytes):
    return [int.from_bytes(p[i:i + 8], "little") for i in range(0, len(p), 8)]


def hash_bytes(p: bytes, seed: int = 0) -> int:
    h = ((FNV0 ^ seed) + len(p)) & M
    for w in _words(p):
        h = _step(h, w)
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & M
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M
    return h ^ (h >> 33)


def collide_same_length(a: bytes, word: bytes, seed: int = 0) -> bytes:
    """Another string of a's length (a multiple of 8, at least 16) with a's hash under ``seed``: a with its last word but one replaced
    by ``word`` (8 bytes, not the one a has) and its last word corrected.  A 16-byte result differs from a in its first word; a
    24-byte one has a's first word."""
    n = len(a)
    assert n >= 16 and n % 8 == 0 and len(word) == 8 and word != a[n - 16:n - 8]
    w = _words(a)
    h = ((FNV0 ^ seed) + n) & M
    for x in w[:-2]:
        h = _step(h, x)
    s, s2 = _step(h, w[-2]), _step(h, int.from_bytes(word, "little"))
    b = a[:n - 16] + word + (w[-1] ^ s ^ s2).to_bytes(8, "little")
    assert b != a and len(b) == n
    return b


def collide_cross_length(a: bytes, seed: int = 0) -> bytes:
    """The 8-byte string with the hash of a (at most 7 bytes) under ``seed``: the lengths enter the start state only, so the single
    word differs by the xor of the two start states."""
    n = len(a)
    assert n <= 7
    h0 = FNV0 ^ seed
    x = ((h0 + n) & M) ^ ((h0 + 8) & M)
    return ((_words(a)[0] if n else 0) ^ x).to_bytes(8, "little")


def collide_printable(a: bytes, rng, seed: int = 0) -> bytes:
    """collide_same_length for a 16-byte a, the first word searched until all 16 bytes are printable ('!' .. '~'): one try in
    (256 / 94) ** 8, a few thousand."""
    assert len(a) == 16
    alphabet = bytes(range(0x21, 0x7f))
    for _ in range(2_000_000):
        word = bytes(rng.choice(alphabet) for _ in range(8))
        if word == a[:8]:
            continue
        b = collide_same_length(a, word, seed)
        if all(0x21 <= c <= 0x7e for c in b):
            return b
    raise AssertionError("no printable collision found")


# ---- the barcode table ----
def table_capacity(n: int) -> int:
    cap = TABLE_MIN_SLOTS
    while cap < 2 * n:
        cap <<= 1
    return cap


def home_slot(tag: bytes, cap: int) -> int:
    return hash_bytes(tag) & 0xffffffff & (cap - 1)


def table_build(barcodes):
    """-> slots (index + 1, 0 = empty): open addressing, linear probing, the first index of a repeated byte string wins."""
    cap = table_capacity(len(barcodes))
    slots = [0] * cap
    for j, b in enumerate(barcodes):
        s = home_slot(b, cap)
        while slots[s] and barcodes[slots[s] - 1] != b:
            s = (s + 1) & (cap - 1)
        if not slots[s]:
            slots[s] = j + 1
    return slots


def probe_path(slots, barcodes, tag: bytes):
    """-> (the slots the lookup of ``tag`` visits, in order; the index found or None)."""
    cap = len(slots)
    s, path = home_slot(tag, cap), []
    while True:
        path.append(s)
        if not slots[s]:
            return path, None
        if barcodes[slots[s] - 1] == tag:
            return path, slots[s] - 1
        s = (s + 1) & (cap - 1)


def tag_with_home(slot: int, cap: int, prefix: bytes, length: int, taken=()) -> bytes:
    """A tag of ``length`` bytes that starts with ``prefix`` and whose home slot in a table of ``cap`` slots is ``slot``: a counter in
    the remaining bytes, searched (about cap tries)."""
    room = length - len(prefix)
    assert room >= 3
    for k in range(1 << 22):
        tag = prefix + k.to_bytes(3, "little") + b"-" * (room - 3)
        if tag not in taken and home_slot(tag, cap) == slot:
            return tag
    raise AssertionError("no tag found")
