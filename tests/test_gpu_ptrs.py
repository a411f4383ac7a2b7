"""GPU tests of qfec_encode_ptrs / qfec_reconstruct_ptrs: shards scattered in device memory, handed
over as a device table of addresses.  The rows of a batch live in one guard-filled pool
(ptrs_common.Pool), in a random permutation of slots, at chosen alignments; the WHOLE pool is compared
with the pool before the call in which only the rows the call must write carry the oracle's bytes, so
one byte stored outside [0, block_size) of a written shard, or anywhere else, fails.  Every case is
also held to qfec_encode / qfec_reconstruct on the same rows gathered contiguously.

Run on an MI355X:  python -m pytest tests/test_gpu_ptrs.py -m gpu -q
"""
import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout
import ptrs_common as pc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")

# templated instances, then two shapes of the runtime-k,m kernels
SHAPES = [(10, 3), (16, 4), (4, 2), (8, 4), (9, 3), (3, 2)]
ALIGN = ["aligned", "residues", "one-data", "one-parity"]
ENC_B = [1, 15, 16, 17, 1000, 1024, 1400]
REC_B = [1, 17, 1000, 1024, 1400]


def whole_pool(t):
    return t.cpu().numpy()


def encode_case(oracle, code, rows, k, m, B, G, mode, seed, alias=None, stream=None):
    """One encode on a pool; returns nothing, asserts everything."""
    n = k + m
    data = pc.batch_bytes(seed, G, k, B)
    for i, j in (alias or {}).items():  # the table repeats an address: the oracle sees the bytes twice
        data.reshape(G * k, B)[i] = data.reshape(G * k, B)[j]
    stale = pc.batch_bytes(seed + 1, G, m, B)  # what the parity shards hold before (the quirk keeps some of it)
    pool = pc.Pool(G * n, B, pc.offsets_for(mode, G, k, m), seed + 2)
    pool.put_all(0, data.reshape(G * k, B))
    pool.put_all(G * k, stale.reshape(G * m, B))
    want = stale.copy()
    oracle.rs_encode(rows, data, want, B)
    expect = pc.Pool(G * n, B, pc.offsets_for(mode, G, k, m), seed + 2)
    expect.host[:] = pool.host
    expect.put_all(G * k, want.reshape(G * m, B))
    t, ptrs = pc.to_device(torch, DEV, pool, alias)
    if stream is None:
        code.encode_ptrs(ptrs, B)
        torch.cuda.synchronize()
        got = whole_pool(t)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            code.encode_ptrs(ptrs, B)
            after = t.clone()  # a dependent kernel on the same stream
        stream.synchronize()
        got = whole_pool(after)
    what = f"({k},{m}) B={B} G={G} {mode}"
    assert np.array_equal(pool.rows_of(got, G * k, G * m), want.reshape(G * m, B)), f"{what}: parity differs from the oracle"
    assert np.array_equal(got, expect.host), f"{what}: a byte outside the parity shards was written"
    # the contiguous call on the same rows
    dd, pp = pc.padded(torch, DEV, data, B), pc.padded(torch, DEV, stale, B)
    code.encode(dd, pp, B)
    torch.cuda.synchronize()
    assert np.array_equal(pp.cpu().numpy()[..., :B], want), f"{what}: qfec_encode differs from the oracle"


@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", SHAPES, ids=[f"{k}-{m}" for k, m in SHAPES])
def test_encode_ptrs(oracle, k, m, mode):
    """G = 7 (the last block is part-empty) at every B of the list: rows of 1 byte, a tail only, no
    tail, one whole column and a tail, a part-filled wave, a full wave, two waves."""
    code = qa.Code.cauchy(k, m)
    for B in ENC_B:
        encode_case(oracle, code, code.rows, k, m, B, 7, mode, 0x9700 + 16 * k + B)


@pytest.mark.parametrize("mode", ["aligned", "one-parity"])
def test_encode_ptrs_many_blocks(oracle, mode):
    """300 groups of one wave each: 75 blocks, so several blocks and more than one XCD are in play."""
    code = qa.Code.cauchy(10, 3)
    encode_case(oracle, code, code.rows, 10, 3, 1024, 300, mode, 0x300)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
@pytest.mark.parametrize("k,m", [(10, 3), (16, 4), (9, 3)], ids=["10-3", "16-4", "9-3"])
def test_encode_ptrs_stale_row_quirk(oracle, k, m, mode):
    """rs.c's column-0 quirk: a parity row whose column-0 coefficient is zero starts from the bytes
    its shard held before.  On the vector body and the byte body, at a B with a tail."""
    rows = oracle.cauchy(k, m).copy()
    rows[1, 0] = 0
    code = qa.Code.from_rows(rows, rs_stale_quirk=True)
    for B in (17, 1000):
        encode_case(oracle, code, rows, k, m, B, 7, mode, 0x5A1E + B + k)


@pytest.mark.parametrize("mode", ["aligned", "residues"])
def test_encode_ptrs_aliased_inputs(oracle, mode):
    """One data shard's address repeated in another group (a shared padding shard): inputs may alias."""
    k, m, G = 10, 3, 7
    code = qa.Code.cauchy(k, m)
    encode_case(oracle, code, code.rows, k, m, 1000, G, mode, 0xA11A, alias={2 * k + 1: 3, 5 * k: 3})


def test_encode_ptrs_on_a_stream(oracle):
    """On a non-default stream, followed by a dependent copy on that stream and a wait for that stream
    alone: no device-wide synchronisation is needed."""
    code = qa.Code.cauchy(10, 3)
    encode_case(oracle, code, code.rows, 10, 3, 1000, 7, "one-data", 0x57E, stream=torch.cuda.Stream())


def reconstruct_case(oracle, code, k, m, B, mode, seed, stream=None):
    n = k + m
    gm = pc.recon_marks(k, m)
    pc.assert_marks_cover(gm, k, m)  # before the GPU is called: the test cannot pass by omission
    G = len(gm)
    assert G == 2 * (m + 3)
    marks = marks_to_rs_layout(gm, k)
    data = pc.batch_bytes(seed, G, k, B)
    data.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    par = pc.batch_bytes(seed + 1, G, m, B)  # not the encode of data: pins which survivors are read
    want = data.copy()
    rc = oracle.rs_reconstruct(code.rows, want, par.copy(), marks, B)
    nfail = pc.oracle_failed(oracle, code.rows, data, par, gm, k, B)
    t_marked = gm.sum(1)
    assert nfail == int((t_marked > m).sum()) and (rc == -1) == (nfail > 0)
    still = (gm[:, :k].sum(1) == 0) | (t_marked > m)
    assert np.array_equal(want[still], data[still])  # the oracle leaves e = 0 and under-determined groups alone
    offs = pc.offsets_for(mode, G, k, m)
    pool = pc.Pool(G * n, B, offs, seed + 2)
    pool.put_all(0, data.reshape(G * k, B))
    pool.put_all(G * k, par.reshape(G * m, B))
    expect = pc.Pool(G * n, B, offs, seed + 2)
    expect.host[:] = pool.host
    expect.put_all(0, want.reshape(G * k, B))
    t, ptrs = pc.to_device(torch, DEV, pool)
    dmarks = torch.from_numpy(marks).to(DEV)
    failed = torch.zeros(1, dtype=torch.int32, device=DEV)
    what = f"({k},{m}) B={B} {mode}"
    if stream is None:
        code.reconstruct_ptrs(ptrs, dmarks, B, failed)
        torch.cuda.synchronize()
        got = whole_pool(t)
    else:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            code.reconstruct_ptrs(ptrs, dmarks, B, failed)
            after = t.clone()
        stream.synchronize()
        got = whole_pool(after)
    assert np.array_equal(pool.rows_of(got, 0, G * k), want.reshape(G * k, B)), f"{what}: data differs from the oracle"
    assert np.array_equal(got, expect.host), f"{what}: a byte outside the marked data shards was written"
    assert int(failed.item()) == nfail, what
    # a second call adds to the counter (the survivors are unchanged, so are the results)
    code.reconstruct_ptrs(ptrs, dmarks, B, failed)
    torch.cuda.synchronize()
    assert int(failed.item()) == 2 * nfail, what
    assert np.array_equal(whole_pool(t), expect.host), what
    # the contiguous call on the same rows
    dd, pp = pc.padded(torch, DEV, data, B), pc.padded(torch, DEV, par, B)
    failed2 = torch.zeros(1, dtype=torch.int32, device=DEV)
    code.reconstruct(dd, pp, dmarks, B, failed2)
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy()[..., :B], want) and int(failed2.item()) == nfail, f"{what}: qfec_reconstruct"


@pytest.mark.parametrize("mode", ALIGN)
@pytest.mark.parametrize("k,m", SHAPES, ids=[f"{k}-{m}" for k, m in SHAPES])
def test_reconstruct_ptrs(oracle, k, m, mode):
    """G = 2 (m + 3) groups with deterministic marks (ptrs_common.recon_marks): every e = 0 .. m,
    parity-only erasures, under-determined groups, m erasures over data and parity; erased rows
    pre-filled with 0x5A; the failed counter equals the oracle's count and accumulates."""
    code = qa.Code.cauchy(k, m)
    for B in REC_B:
        reconstruct_case(oracle, code, k, m, B, mode, 0x4EC0 + 16 * k + B)


def test_reconstruct_ptrs_on_a_stream(oracle):
    code = qa.Code.cauchy(16, 4)
    reconstruct_case(oracle, code, 16, 4, 1400, "one-parity", 0x57F, stream=torch.cuda.Stream())


def test_reconstruct_ptrs_null_failed_counter(oracle):
    """d_failed may be NULL: the same bytes, nothing counted."""
    k, m, B = 10, 3, 1000
    code = qa.Code.cauchy(k, m)
    gm = pc.recon_marks(k, m)
    G, n = len(gm), k + m
    marks = marks_to_rs_layout(gm, k)
    data = pc.batch_bytes(0xF00, G, k, B)
    data.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    par = pc.batch_bytes(0xF01, G, m, B)
    want = data.copy()
    oracle.rs_reconstruct(code.rows, want, par.copy(), marks, B)
    pool = pc.Pool(G * n, B, pc.offsets_for("aligned", G, k, m), 3)
    pool.put_all(0, data.reshape(G * k, B))
    pool.put_all(G * k, par.reshape(G * m, B))
    t, ptrs = pc.to_device(torch, DEV, pool)
    code.reconstruct_ptrs(ptrs, torch.from_numpy(marks).to(DEV), B)
    torch.cuda.synchronize()
    assert np.array_equal(pool.rows_of(whole_pool(t), 0, G * k), want.reshape(G * k, B))
