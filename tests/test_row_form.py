"""The row form that kernels K10 and K14 read (CSR rows, or one value for a row that holds it at every state) is checked by
one function, check_row_form of csrc/cmdp_batch.h, for both cmdp_extended_vi and cmdp_vi_discounted_model: every refusal
through either entry point, before any device is touched, and the global row index of a fault in a ragged batch."""
import numpy as np
import pytest

import helpers_model_vi as H
from colosseum_amd import _lib as L

ENTRIES = ("extended_vi", "vi_discounted_model")


def call(entry, args, **kw):
    """(rc, message) of the entry point on the packed arguments of helpers_model_vi.pack, `kw` replacing some of them."""
    lib = L.load()
    count = len(args["n_states"])
    nr = int((args["n_states"].astype(np.int64) * args["n_actions"]).sum())
    a = dict(args, **kw)
    model = [L.ptr(a[k]) for k in ("n_states", "n_actions", "ptr", "col", "val", "uni", "R")]
    Q, V = np.zeros(nr, np.float32), np.zeros(int(args["n_states"].sum()), np.float32)
    sweeps, status = np.zeros(count, np.int64), np.zeros(count, np.int32)
    if entry == "extended_vi":
        beta, r_max, span = np.zeros(nr), np.ones(count), np.zeros(count)
        rc = lib.cmdp_extended_vi(count, *model, L.ptr(beta), L.ptr(beta), L.ptr(r_max), 1e-3, 10,
                                  L.ptr(Q), L.ptr(V), L.ptr(span), L.ptr(sweeps), L.ptr(status))
    else:
        scheme = np.zeros(count, np.int32)
        rc = lib.cmdp_vi_discounted_model(count, *model, 0.99, 1e-3, L.SCHEME_AUTO, H.SIZE_THRESHOLD, H.DENSITY_THRESHOLD, 10,
                                          L.ptr(Q), L.ptr(V), L.ptr(sweeps), L.ptr(scheme), L.ptr(status))
    return rc, lib.cmdp_last_error().decode()


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_form_refusals(entry):
    args = H.pack([H.make_fixture(3, 2, "state_0", 1)])   # rows 0 and 1 uniform, rows 2 .. 5 CSR

    def invalid(word, **kw):
        rc, msg = call(entry, args, **kw)
        assert rc == L.ERR_INVALID and word in msg, (kw, rc, msg)

    invalid("null argument", ptr=None)
    invalid("null argument", R=None)
    invalid("null csr_col / csr_val", col=None)
    invalid("null csr_col / csr_val", val=None)
    bad = args["ptr"].copy(); bad[0] = 1
    invalid("csr_ptr[0] = 1, not 0", ptr=bad)
    invalid("csr_ptr[0]", ptr=np.ones(7, np.int64))
    bad = args["ptr"].copy(); bad[3] = bad[2] - 1
    invalid("csr_ptr decreases at row 2", ptr=bad)
    multi = next(r for r in range(2, 6) if args["ptr"][r + 1] - args["ptr"][r] >= 2)
    k0 = int(args["ptr"][multi])
    bad = args["col"].copy(); bad[k0 + 1] = bad[k0]
    invalid(f"csr_col of row {multi} is not ascending within [0, 3)", col=bad)
    for c in (3, -1):
        bad = args["col"].copy(); bad[k0] = c
        invalid(f"csr_col of row {multi}", col=bad)
    for v in (-0.5, -1.0, np.inf, np.nan):
        bad = args["val"].copy(); bad[1] = v
        invalid("csr_val[1]", val=bad)
    for v in (np.inf, np.nan):
        bad = args["R"].copy(); bad[4] = v
        invalid("rewards[4]", R=bad)
    for v in (-0.5, np.inf, np.nan):
        bad = args["uni"].copy(); bad[0] = v
        invalid("uniform[0]", uni=bad)
    invalid("uniform[0]", uni=np.full(6, -0.5, np.float32))
    bad = args["uni"].copy(); bad[multi] = 0.25   # a uniform value on a row that has entries
    invalid(f"uniform[{multi}] = 0.25: must be finite > 0 on a row without CSR entries", uni=bad)
    # one entry per row, as the smallest malformed models are written by hand
    one = np.arange(7, dtype=np.int64)
    z, no_uni = np.zeros(6, np.int32), np.zeros(6, np.float32)
    invalid("csr_col of row 0", ptr=one, uni=no_uni, col=np.full(6, 3, np.int32), val=np.ones(6, np.float32))
    invalid("csr_val[0]", ptr=one, uni=no_uni, col=z, val=np.full(6, -1, np.float32))
    invalid("uniform[0]", ptr=one, uni=np.full(6, 1 / 3, np.float32), col=z, val=np.ones(6, np.float32))


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_fault_in_a_ragged_batch_carries_the_global_row(entry):
    """S = (3, 2), A = (2, 3): the second instance's rows are 6 .. 11 and its columns lie within [0, 2)."""
    args = H.pack([H.make_fixture(3, 2, "state_0", 1), H.make_fixture(2, 3, "no_uniform", 2)])
    assert len(args["R"]) == 12 and args["ptr"][12] > args["ptr"][11]
    last = int(args["ptr"][12]) - 1   # the last entry of row 11
    bad = args["col"].copy(); bad[last] = 2   # a column of the first instance's range
    assert call(entry, args, col=bad) == (L.ERR_INVALID, "csr_col of row 11 is not ascending within [0, 2)")
    bad = args["val"].copy(); bad[last] = -1
    assert call(entry, args, val=bad) == (L.ERR_INVALID, f"csr_val[{last}] = -1 is not a finite probability >= 0")
    bad = args["R"].copy(); bad[11] = np.nan
    assert call(entry, args, R=bad) == (L.ERR_INVALID, "rewards[11] is not finite")
    bad = args["uni"].copy(); bad[11] = 0.5
    assert call(entry, args, uni=bad) == (L.ERR_INVALID, "uniform[11] = 0.5: must be finite > 0 on a row without CSR entries")
    bad = args["ptr"].copy(); bad[11] = bad[12] + 1
    assert call(entry, args, ptr=bad) == (L.ERR_INVALID, "csr_ptr decreases at row 11")
