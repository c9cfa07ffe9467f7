"""GPU: the batched Huffman coders (cst_huffman_encode_batch / cst_huffman_decode_batch) against the reference's doc vectors and
the plain-Python restatement of tests/huffman_ref.py."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import huffman_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
DOC = json.loads((ROOT / "tests" / "golden" / "huffman_vectors.json").read_text())["doc_examples"]


@pytest.fixture(scope="module")
def B():
    from constriction_amd import batched
    return batched


def expected(nodes, sym, semantics):
    codes = R.suffix_codewords(nodes) if semantics == "stack" else R.prefix_codewords(nodes)
    enc = R.stack_encode if semantics == "stack" else R.queue_encode
    return [enc(nodes, row, codes) for row in sym.tolist()]


def check_batch(batch, want):
    words, n_words, status = batch.to_numpy()
    n_bits = batch.n_bits.cpu().numpy()
    assert (status == 0).all()
    for s, (w, bits) in enumerate(want):
        assert n_bits[s] == bits, s
        assert n_words[s] == len(w), s
        assert words[s, : n_words[s]].tolist() == w, s


def test_doc_vectors(B):
    cb = B.HuffmanCodebook.from_probabilities(np.array(DOC["probabilities"], dtype=np.float32))
    msg = torch.tensor([DOC["message"]], dtype=torch.int32, device="cuda")
    q = B.huffman_encode(msg, cb, "queue")
    assert q.stream(0).tolist() == DOC["queue"]["words"] and int(q.n_bits[0]) == DOC["queue"]["bitrate"]
    assert B.last_kernel() == "huffman_encode_kernel"
    s = B.huffman_encode(msg, cb, "stack")
    st = DOC["stack_encoded_in_reverse"]
    assert s.stream(0).tolist() == st["words"] and int(s.n_bits[0]) == st["bitrate"]
    for batch in (q, s):
        dec, status = B.huffman_decode(batch, cb, len(DOC["message"]))
        assert B.last_kernel() == "huffman_decode_kernel"
        assert status.tolist() == [0] and dec[0].tolist() == DOC["message"]


def random_codebook(B, rng, n, f32=False):
    p = rng.dirichlet(np.ones(n) * 0.5)
    p = p.astype(np.float32) if f32 else p
    return B.HuffmanCodebook.from_probabilities(p), p


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
@pytest.mark.parametrize("n_streams,n_per", [(1, 50), (255, 37), (257, 64), (65537, 2), (70000, 3), (300, 0), (300, 1)])
def test_random_batches(B, semantics, dtype, n_streams, n_per):
    rng = np.random.default_rng(n_streams * 131 + n_per)
    cb, p = random_codebook(B, rng, 23 if dtype == torch.uint8 else 300, f32=n_per % 2 == 1)
    sym = rng.choice(p.size, size=(n_streams, n_per), p=np.asarray(p, np.float64) / np.sum(p, dtype=np.float64))
    sym_t = torch.from_numpy(sym.astype(np.uint8 if dtype == torch.uint8 else np.int32)).cuda()
    batch = B.huffman_encode(sym_t, cb, semantics)
    check_batch(batch, expected(cb.nodes.tolist(), sym, semantics))
    dec, status = B.huffman_decode(batch, cb, n_per, dtype=dtype)
    assert (status.cpu().numpy() == 0).all()
    assert np.array_equal(dec.cpu().numpy().astype(np.int64), sym)


def dyadic(n):
    """probabilities 2^-1, 2^-2, ..., 2^-(n-1), 2^-(n-1): codeword lengths 1 .. n-1, the longest n-1"""
    return np.array([2.0 ** -i for i in range(1, n)] + [2.0 ** -(n - 1)])


@pytest.mark.parametrize("longest,enc_kernel", [(32, "huffman_encode_kernel"), (33, "huffman_encode_long_kernel"),
                                                (300, "huffman_encode_long_kernel")])
@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_long_codes(B, longest, enc_kernel, semantics):
    cb = B.HuffmanCodebook.from_probabilities(dyadic(longest + 1))
    assert max(len(c) for c in R.suffix_codewords(cb.nodes.tolist())) == longest
    rng = np.random.default_rng(longest)
    n_streams, n_per = 300, 40
    sym = rng.integers(0, longest + 1, (n_streams, n_per))
    sym[:, :3] = longest                                     # the longest codewords in every stream
    batch = B.huffman_encode(torch.from_numpy(sym.astype(np.int32)).cuda(), cb, semantics)
    assert B.last_kernel() == enc_kernel
    check_batch(batch, expected(cb.nodes.tolist(), sym, semantics))
    dec, status = B.huffman_decode(batch, cb, n_per)
    assert B.last_kernel() == "huffman_decode_long_kernel"
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_words_sized_by_max_words(B, semantics):
    cb = B.HuffmanCodebook.from_probabilities(dyadic(41))
    for n_per in (0, 1, 7, 100):
        sym = torch.full((3, n_per), 40, dtype=torch.int32, device="cuda")   # every codeword at the longest
        stride = cb.max_words(n_per, semantics)
        batch = B.huffman_encode(sym, cb, semantics, stride=stride)
        assert batch.status.tolist() == [0, 0, 0]
        need = int(batch.n_words[0])
        assert need <= stride
        if need > 0:
            small = B.huffman_encode(sym, cb, semantics, stride=need - 1)
            assert small.status.tolist() == [2, 2, 2] and small.n_words.tolist() == [0, 0, 0]


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_compacted_words_decode(B, semantics):
    rng = np.random.default_rng(5)
    cb, p = random_codebook(B, rng, 50)
    sym = rng.integers(0, 50, (1000, 33))
    batch = B.huffman_encode(torch.from_numpy(sym.astype(np.int32)).cuda(), cb, semantics)
    packed, offsets = B.compact(batch)
    dec, status = B.huffman_decode((packed, batch.n_words), cb, 33, semantics=semantics, offsets=offsets)
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


@pytest.mark.parametrize("semantics", ["stack", "queue"])
@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_impossible_symbols(B, semantics, dtype):
    cb = B.HuffmanCodebook.from_probabilities(np.array([0.5, 0.25, 0.25]))
    sym = np.ones((5, 20), dtype=np.int64)
    sym[0, 0] = 3
    sym[1, 10] = 200
    sym[2, 19] = 3
    if dtype == torch.int32:
        sym[3, 5] = -1
    batch = B.huffman_encode(torch.from_numpy(sym.astype(np.uint8 if dtype == torch.uint8 else np.int32)).cuda(), cb, semantics)
    bad = [1, 1, 1, 1 if dtype == torch.int32 else 0, 0]
    assert batch.status.tolist() == bad
    assert batch.n_words.tolist() == [0 if b else int(batch.n_words[4]) for b in bad]


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_prefix_and_out_of_data(B, semantics):
    rng = np.random.default_rng(9)
    cb, p = random_codebook(B, rng, 40)
    nodes = cb.nodes.tolist()
    sym = rng.integers(0, 40, (200, 30))
    batch = B.huffman_encode(torch.from_numpy(sym.astype(np.int32)).cuda(), cb, semantics)
    dec, status = B.huffman_decode(batch, cb, 12)
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym[:, :12])
    dec, status = B.huffman_decode(batch, cb, 60)
    words, n_words, _ = batch.to_numpy()
    dec, status = dec.cpu().numpy(), status.cpu().numpy()
    for s in range(200):
        want, ood = R.decode(nodes, words[s, : n_words[s]].tolist(), 60, semantics)
        assert status[s] == (4 if ood else 0), s
        assert dec[s, : len(want)].tolist() == want and (dec[s, len(want):] == 0).all()


def test_stack_without_seal_is_invalid(B):
    cb = B.HuffmanCodebook.from_probabilities(np.array([0.5, 0.5]))
    words = torch.tensor([[5, 0], [5, 7]], dtype=torch.int32, device="cuda")
    n_words = torch.tensor([2, 0], dtype=torch.int32, device="cuda")
    dec, status = B.huffman_decode((words, n_words), cb, 1, semantics="stack")
    assert status.tolist() == [3, 3]
    from constriction_amd import _native as N
    with pytest.raises(N.BackendError, match="cst_huffman_decode_batch: invalid argument"):     # 300 symbols do not fit uint8
        B.huffman_decode((words, n_words), B.HuffmanCodebook.from_probabilities(np.ones(300)), 1, semantics="stack",
                         dtype=torch.uint8)


def _call_encode(cb, sem, sym, cont, stride):
    from constriction_amd import _native as N
    n_streams, n_per = sym.shape
    words = torch.zeros((n_streams, stride), dtype=torch.int32, device="cuda")
    n_words = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    sym = sym.contiguous()
    N.check(N.lib().cst_huffman_encode_batch(cb._h, sem, C.c_void_p(sym.data_ptr()), 4, n_streams, n_per, C.c_void_p(words.data_ptr()),
                                             stride, C.c_void_p(n_words.data_ptr()), None, C.c_void_p(cont.data_ptr()),
                                             C.c_void_p(status.data_ptr()), None))
    assert (status.cpu().numpy() == 0).all()
    w, n = words.cpu().numpy().view(np.uint32), n_words.cpu().numpy()
    return [w[s, : n[s]].tolist() for s in range(n_streams)]


def _call_decode(cb, sem, words_rows, n_per, cont):
    from constriction_amd import _native as N
    n_streams = len(words_rows)
    stride = max(1, max(len(r) for r in words_rows))
    w = np.zeros((n_streams, stride), dtype=np.uint32)
    for s, r in enumerate(words_rows):
        w[s, : len(r)] = r
    dw = torch.from_numpy(w.view(np.int32)).cuda()
    nw = torch.tensor([len(r) for r in words_rows], dtype=torch.int32, device="cuda")
    out = torch.zeros((n_streams, n_per), dtype=torch.int32, device="cuda")
    n_out = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    status = torch.zeros(n_streams, dtype=torch.int32, device="cuda")
    N.check(N.lib().cst_huffman_decode_batch(cb._h, sem, C.c_void_p(dw.data_ptr()), None, stride, dw.numel(), C.c_void_p(nw.data_ptr()),
                                             C.c_void_p(out.data_ptr()), 4, n_streams, n_per, C.c_void_p(cont.data_ptr()),
                                             C.c_void_p(n_out.data_ptr()), C.c_void_p(status.data_ptr()), None))
    assert (status.cpu().numpy() == 0).all()
    return out.cpu().numpy(), n_out.cpu().numpy()


@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_two_continued_calls_equal_one(B, semantics):
    from constriction_amd import _native as N
    sem = N.HUFFMAN_STACK if semantics == "stack" else N.HUFFMAN_QUEUE
    rng = np.random.default_rng(77)
    cb, p = random_codebook(B, rng, 60)
    n_streams, n_per, h = 100, 50, 17
    sym = torch.from_numpy(rng.integers(0, 60, (n_streams, n_per)).astype(np.int32)).cuda()
    one = B.huffman_encode(sym, cb, semantics)
    cont = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
    stride = cb.max_words(n_per, semantics)
    # a stack codes a row back to front: the second half goes on first
    first, second = (sym[:, h:], sym[:, :h]) if semantics == "stack" else (sym[:, :h], sym[:, h:])
    w1 = _call_encode(cb, sem, first, cont, stride)
    w2 = _call_encode(cb, sem, second, cont, stride)
    c = cont.cpu().numpy()
    partial, nb = c & 0xFFFFFFFF, c >> 32
    for s in range(n_streams):
        tail = [int(partial[s] | (1 << int(nb[s])))] if semantics == "stack" else ([int(partial[s])] if nb[s] else [])
        assert w1[s] + w2[s] + tail == one.stream(s).tolist(), s
    # and the decoder: half the symbols, then the rest from where it stopped
    rows = [one.stream(s).tolist() for s in range(n_streams)]
    if semantics == "stack":
        tops = [r[-1].bit_length() - 1 for r in rows]
        cont = torch.tensor([(r[-1] ^ (1 << t)) | (t << 32) for r, t in zip(rows, tops)], dtype=torch.int64, device="cuda")
        rows = [r[:-1] for r in rows]
    else:
        cont = torch.zeros(n_streams, dtype=torch.int64, device="cuda")
    d1, left = _call_decode(cb, sem, rows, h, cont)
    if semantics == "stack":
        rows = [r[: int(k)] for r, k in zip(rows, left)]
    d2, _ = _call_decode(cb, sem, rows, n_per - h, cont)
    assert np.array_equal(np.concatenate([d1, d2], axis=1), sym.cpu().numpy())


@pytest.mark.parametrize("n_sym", [8193, 65536])
@pytest.mark.parametrize("semantics", ["stack", "queue"])
def test_large_alphabets(B, n_sym, semantics):
    """past 8192 symbols the encoder reads its codeword table from global memory; 65 536 = CST_HUFFMAN_MAX_SYMBOLS"""
    rng = np.random.default_rng(n_sym)
    p = rng.random(n_sym) + 1e-3
    cb = B.HuffmanCodebook.from_probabilities(p)
    nodes = cb.nodes.tolist()
    assert nodes == R.tree(p, False)
    sym = rng.integers(0, n_sym, (130, 77))
    sym[:, 0] = n_sym - 1
    batch = B.huffman_encode(torch.from_numpy(sym.astype(np.int32)).cuda(), cb, semantics)
    check_batch(batch, expected(nodes, sym, semantics))
    dec, status = B.huffman_decode(batch, cb, 77)
    assert (status.cpu().numpy() == 0).all() and np.array_equal(dec.cpu().numpy(), sym)


def test_more_than_65536_symbols_are_rejected(B):
    from constriction_amd import _native as N
    nodes = B.huffman_tree(np.ones(65537))
    with pytest.raises(ValueError):
        B.HuffmanCodebook(nodes)
    h = C.c_void_p()
    assert N.lib().cst_huffman_codebook_create(nodes.ctypes.data, 65537, None, C.byref(h)) == N.CST_ERR_INVALID_ARGUMENT
    assert not h.value


def test_reused_out_must_match_the_batch(B):
    cb = B.HuffmanCodebook.from_probabilities(np.array([0.5, 0.5]))
    sym = torch.zeros((10, 5), dtype=torch.int32, device="cuda")
    out = B.huffman_encode(sym, cb, "queue")
    assert B.huffman_encode(sym, cb, "stack", out=out) is out and out.semantics == "stack"
    with pytest.raises(ValueError):
        B.huffman_encode(torch.zeros((11, 5), dtype=torch.int32, device="cuda"), cb, "stack", out=out)
    with pytest.raises(TypeError):
        B.huffman_decode((out.words, out.n_words.to(torch.int64)), cb, 5, semantics="stack")
