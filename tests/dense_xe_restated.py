"""Cross-entropy caption training over every matched object of a scene restated in numpy: the
specification of ``spacap_dense_xe_targets_i64`` (csrc/dense_xe.hip), with the corpus and the key arrays both test modules run
through it.  Not a test module.  The selection is tests/scene_scst_restated.py's, the loss tests/losses_restated.py's with rows
in the place of scenes.

The draw.  Group g = b M + m with key row ``key`` holding n references: ``seed = make_seed(host word, device word)`` =
host + device * 0x9E3779B97F4A7C15 mod 2^64 as (low, high) halves (csrc/dropout.hpp), ``h = hash32(g, seed)`` -- murmur3's fmix32
over the index mixed with both halves --, ``j0 = (h * n) >> 32``; row s < r takes reference ``key_ref_off[key] + (j0 + s) % n``
when s < n and is empty otherwise (and wholly empty for a key outside 0..nkeys-1 or n = 0).

The row.  A sentence of len ids becomes T ids: its ids then zeros (len <= T) or its first T - 1 ids then eos (len > T); an id
outside 0..n_vocab-1 becomes unk.  An empty row is sos eos and zeros.  ``sentence_row`` states the same for one sentence by the
reference's own road (lib/dataset.py:97-108): the words trimmed to 30, sos / eos around them, word2idx with unk, zeros to 32."""
import collections
import functools

import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B97F4A7C15
T_IDS = 32                   # MAX_DES_LEN + 2
MAX_DES_LEN = 30

Targets = collections.namedtuple("Targets", "tok ids ref good length")


def make_seed(seed, seed_dev=None):
    """(low, high) halves of the 64-bit seed; ``seed_dev`` None: no device word"""
    s = (int(seed) + (int(seed_dev) * GOLDEN if seed_dev is not None else 0)) & M64
    return s & M32, s >> 32


def hash32(idx, seed):
    lo, hi = seed
    idx = int(idx) & M64
    h = (idx & M32) ^ lo
    h = (h + (((idx >> 32) ^ hi) * 0x9E3779B1)) & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def first_reference(g, n, seed):
    """j0 of group g over n >= 1 references"""
    return (hash32(g, seed) * int(n)) >> 32


def chosen(g, n, r, seed):
    """the r reference indices (inside the key's n) of group g, -1 for an empty row"""
    if n <= 0:
        return [-1] * r
    j0 = first_reference(g, n, seed)
    return [(j0 + s) % n if s < n else -1 for s in range(r)]


def id_row(sent, T, n_vocab, unk, eos):
    """the T ids of a sentence given as ids, and its target length"""
    sent = [int(t) if 0 <= int(t) < n_vocab else unk for t in sent]
    row = sent[:T - 1] + [eos] if len(sent) > T else sent
    return row + [0] * (T - len(row)), max(min(len(sent), T) - 1, 0)


def targets(key, ref_tok, ref_off, ref_len, key_ref_off, n_vocab, unk, sos, eos, r, T, seed, seed_dev=None):
    """what spacap_dense_xe_targets_i64 writes for ``key`` (B, M)"""
    key = np.asarray(key)
    G, nkeys = key.size, len(key_ref_off) - 1
    sd = make_seed(seed, seed_dev)
    out = Targets(np.zeros((G * r, T + 1), np.int64), np.zeros((G * r, T), np.int64), np.full(G * r, -1, np.int32),
                  np.zeros(G * r, np.uint8), np.zeros(G * r, np.int32))
    out.tok[:, 0] = 1
    for g, k in enumerate(key.reshape(-1)):
        n = int(key_ref_off[k + 1] - key_ref_off[k]) if 0 <= k < nkeys else 0
        for s, j in enumerate(chosen(g, n, r, sd)):
            row = g * r + s
            if j < 0:
                out.ids[row, :2] = (sos, eos)
            else:
                ref = int(key_ref_off[k]) + j
                sent = ref_tok[ref_off[ref]:ref_off[ref] + ref_len[ref]]
                out.ids[row], out.length[row] = id_row(sent, T, n_vocab, unk, eos)
                out.ref[row], out.good[row] = ref, 1
    out.tok[:, 1:] = out.ids
    return out


def sentence_row(sentence, word2idx):
    """One corpus sentence ("sos w1 ... wn eos") as the reference's dataset lays its words out (lib/dataset.py:97-108): split,
    the words trimmed to MAX_DES_LEN, sos / eos, word2idx with unk for a KeyError, zeros to MAX_DES_LEN + 2."""
    words = sentence.split()
    assert words[0] == "sos" and words[-1] == "eos"
    tokens = ["sos"] + words[1:-1][:MAX_DES_LEN] + ["eos"]
    labels = np.zeros(MAX_DES_LEN + 2, np.int64)
    for i, t in enumerate(tokens):
        try:
            labels[i] = word2idx[t]
        except KeyError:
            labels[i] = word2idx["unk"]
    return labels


# ---- the hand-built corpus of both test modules ----------------------------------------------------------------------------
N_VOCAB = 20
W2I = {w: i for i, w in enumerate(["pad_", "unk", "sos", "eos"] + [f"w{i}" for i in range(4, N_VOCAB)])}
UNK, SOS, EOS = 1, 2, 3
REFS_PER_KEY = (0, 1, 2, 3, 7, 9)
# the words of chosen sentences: (key, reference) -> number of words; 30 / 31 / 62 words are 32 / 33 / 64 ids
WORDS = {(1, 0): 30, (2, 1): 31, (3, 2): 62, (4, 0): 1, (4, 3): 29, (5, 8): 45}
HOST_SEED = 0x1234567890ABCDEF
DEVICE_WORDS = (None, 0, 2 ** 33 + 5)
TARGET_CASES = ((1, 1, 1), (3, 5, 1), (2, 16, 3), (2, 4, 8), (5, 128, 2))


@functools.lru_cache(maxsize=None)
def hand_corpus():
    """({key: [sentence, ...]}, word2idx): keys with 0, 1, 2, 3, 7 and 9 references; sentences of 32, 33 and 64 ids; words
    outside the vocabulary first, last and adjacent ("x..": the corpus numbers them from N_VOCAB upward, so the first of them
    carries the id N_VOCAB and the last new one the largest id); the last vocabulary word w19 = N_VOCAB - 1."""
    rng = np.random.default_rng(70)
    corpus, fresh = {}, 0
    for k, n in enumerate(REFS_PER_KEY):
        sents = []
        for j in range(n):
            nw = WORDS.get((k, j), int(rng.integers(2, 28)))
            words = [f"w{int(t)}" for t in rng.integers(4, N_VOCAB, nw)]
            words[nw // 2] = f"w{N_VOCAB - 1}"
            if (k + j) % 2 == 0:                      # a new word outside the vocabulary in front
                words[0] = f"x{fresh}"
                fresh += 1
            if (k + j) % 3 == 0 and nw >= 2:          # ... and one at the end, adjacent to the first in a two-word sentence
                words[-1] = f"x{fresh}"
                fresh += 1
            if j == 1 and nw >= 6:                    # two adjacent ones, the second seen before
                words[3:5] = [f"x{fresh}", "x0"]
                fresh += 1
            sents.append("sos " + " ".join(words) + " eos")
        corpus["k%d" % k] = sents
    corpus["k5"][-1] = "sos " + " ".join(corpus["k5"][-1].split()[1:-2] + [f"x{fresh}"]) + " eos"     # the largest id, last word
    return corpus, dict(W2I)


@functools.lru_cache(maxsize=None)
def key_array(case):
    """key (B, M) int32 of a case: the six keys and -1 mixed; where B > 1 the last scene has no key at all, where B > 2 key 4
    sits in scenes 0 and 1; the largest case holds one key behind the table (no row: its group is empty)."""
    B, M, r = case
    rng = np.random.default_rng(900 + 17 * B + M)
    key = rng.integers(-1, len(REFS_PER_KEY), (B, M)).astype(np.int32)
    if B * M == 1:
        key[0, 0] = 5
    if M >= 4:
        key[0, :4] = (0, 5, -1, 1)
    if B > 1:
        key[B - 1] = -1
    if B > 2:
        key[0, M - 1] = key[1, 0] = 4
    if M == 128:
        key[2, 7] = len(REFS_PER_KEY)
    key.setflags(write=False)
    return key
