"""The addNewWords decision loop (resolve_body.cuh) on every route, entry and producer: the designed frames of tests/resolve_inputs.py -- whose routes,
sweeps and seams tests/test_resolve_inputs.py proves on the CPU -- through lcd_quantize (resolve_kernel), lcd_frame_dev on a plain handle
(frame_tail_body) and on a pipelined handle (frame_resolve_part), each twice in a row, on f32 handles in every 2-NN mode with the 300-row vocabulary
(the matrix-core filter's re-rank leaves bit rows, compact lists and counts) and with its first 200 rows (the exact scan and launch_selfdist leave bit
rows only), on a 128-float handle (the wide filter finds the neighbours, launch_selfdist leaves the bit rows), and on u8 handles with the Hamming analogues (the fused Hamming merge).  Every comparison is exact: word ids after
the suite's mapping and n_new against the oracle's addNewWords, and the entries against each other.

Where the re-rank is the producer the exact redo must stay inside knn_last_fallback_queries <= q // 4 (the inputs are built for that: every
descriptor is certified on the CPU), so a broken list cannot hide behind it; one input leaves the cap on purpose -- a cluster on a run of identical
rows -- to show that a redone query's candidate information is rederived."""
import numpy as np
import pytest
import torch  # before liblcd_hip.so is loaded: one HIP runtime per process (rtabmap_amd/capi.py)

import resolve_inputs as I

pytestmark = pytest.mark.gpu

F32_HANDLES = [("f32", 64, mode, rows) for mode in ("valu", "bf16", "f16", "mfma32") for rows in (300, 200)] + [("f32", 128, "bf16", 300)]
U8_HANDLES = [("u8", 32, "default", 300), ("u8", 32, "hamming_mfma", 300)]

_EXPECTED = {}


def _case(dtype, dim, rows, name):
    """(vocab, ids, frame, nndr, the oracle's word ids) of one input on one kind of handle -- computed once, shared, never written to"""
    key = (dtype, dim, rows, name)
    if key not in _EXPECTED:
        import oracle as O
        vocab, ids, frame, nndr = (I.u8_all_inputs() if dtype == "u8" else dict(I.all_inputs(), redo=I.redo))[name]()
        if vocab.shape[0] > rows:
            vocab, ids = vocab[:rows], ids[:rows]
        if dtype == "f32" and dim != I.DIM:
            vocab, frame = I.widen(vocab, dim), I.widen(frame, dim)
        m = O.OracleVWDictionary(strategy=O.kNNBruteForce, nndr=nndr)
        for i, r in zip(ids, vocab):
            m.add_word(int(i), r)
        m.update()
        exp = m.add_new_words(frame, 1)
        m.close()
        _EXPECTED[key] = (vocab, ids, frame, nndr, exp)
    return _EXPECTED[key]


class _Handles:
    """a plain and a pipelined handle per vocabulary the inputs name (300 or 200 rows, one row, none)"""

    def __init__(self, dtype, dim, mode):
        self.dtype, self.dim, self.mode, self.by_rows = dtype, dim, mode, {}

    def get(self, vocab, ids):
        import rtabmap_amd
        key = (vocab.shape[0], vocab.tobytes()[:4096])
        if key not in self.by_rows:
            pair = []
            for pipeline in (False, True):
                eng = rtabmap_amd.Engine(self.dtype, self.dim, sig_capacity=64, knn_mode=self.mode, pipeline=pipeline)
                if vocab.shape[0]:
                    eng.vocab_append(vocab, ids)
                pair.append(eng)
            self.by_rows[key] = pair
        return self.by_rows[key]

    def close(self):
        for pair in self.by_rows.values():
            for eng in pair:
                eng.close()


def _frame_dev_twice(eng, frame, nndr):
    """two consecutive lcd_frame_dev calls (sig_id 0: the dictionary and the index stay as they are), then one synchronisation"""
    q = frame.shape[0]
    d = torch.from_numpy(frame).cuda()
    d_words = torch.full((2, q), 12345, dtype=torch.int32, device="cuda")
    for k in range(2):
        eng.frame_dev(d.data_ptr(), q, 0, 10.0, d_words[k].data_ptr(), 0, 0, incremental=True, new_words_compared=True, nndr=nndr)
    eng.synchronize()
    return d_words.cpu().numpy()


def _run_input(handles, dtype, dim, mode, rows, name, behind_filter):
    vocab, ids, frame, nndr, exp = _case(dtype, dim, rows, name)
    n, q = len(ids), frame.shape[0]
    plain, piped = handles.get(vocab, ids)
    got, n_new = plain.quantize(frame, incremental=True, new_words_compared=True, nndr=nndr)
    redone = plain.stats()["knn_last_fallback_queries"]
    assert np.where(got < 0, n - got, got).tolist() == exp, "%s: lcd_quantize differs from the oracle" % name
    assert n_new == len({w for w in exp if w > n}), name
    again, n_again = plain.quantize(frame, incremental=True, new_words_compared=True, nndr=nndr)
    assert again.tolist() == got.tolist() and n_again == n_new, "%s: the second lcd_quantize differs from the first" % name
    for what, eng in (("plain", plain), ("pipelined", piped)):
        w = _frame_dev_twice(eng, frame, nndr)
        assert w[0].tolist() == got.tolist(), "%s: lcd_frame_dev (%s handle) differs from lcd_quantize" % (name, what)
        assert w[1].tolist() == got.tolist(), "%s: the second lcd_frame_dev (%s handle) differs" % (name, what)
    filtered = behind_filter and n >= 256                                 # the matrix-core filter and its certificate ran: the cap applies
    lists = filtered and dim == 64                                    # ... and its re-rank left lists and counts (rows of 64 floats only)
    print("%-20s q %4d rows %3d new %3d redone exactly %d%s" % (name, q, n, n_new, redone, " (filter + re-rank%s)" % (": lists" if lists else "") if filtered else ""))
    return redone, filtered, q


@pytest.mark.parametrize("dtype,dim,mode,rows", F32_HANDLES)
def test_every_designed_frame_on_every_entry_f32(oracle, dtype, dim, mode, rows):
    handles = _Handles(dtype, dim, mode)
    total = 0
    for name in I.all_inputs():
        redone, filtered, q = _run_input(handles, dtype, dim, mode, rows, name, behind_filter=mode != "valu")
        if filtered:
            assert redone <= q // 4, "%s: %d of %d queries went to the exact redo" % (name, redone, q)
            total += redone
    print("queries redone exactly over all inputs behind the filter:", total)
    handles.close()


@pytest.mark.parametrize("dtype,dim,mode,rows", U8_HANDLES)
def test_every_designed_frame_on_every_entry_hamming(oracle, dtype, dim, mode, rows):
    handles = _Handles(dtype, dim, mode)
    for name in I.u8_all_inputs():
        _run_input(handles, dtype, dim, mode, rows, name, behind_filter=False)
    handles.close()


@pytest.mark.parametrize("mode", ["bf16", "f16", "mfma32"])
def test_a_cluster_on_identical_rows_is_redone_with_its_candidate_information(oracle, mode):
    """seven descriptors 9 or 10 from 42 identical rows: the certificate rejects each (asserted on the CPU), the exact redo stands in for the re-rank and
    must leave their bit rows, lists and counts -- the cluster's first is new, the six behind it match it through lists of 1 to 4 and bit rows of 5 and 6"""
    handles = _Handles("f32", 64, mode)
    redone, filtered, q = _run_input(handles, "f32", 64, mode, 300, "redo", behind_filter=True)
    exp = _case("f32", 64, 300, "redo")[4]
    assert filtered and redone >= 7 > q // 4
    assert exp[4] > 300 and exp[4:11] == [exp[4]] * 7
    handles.close()
