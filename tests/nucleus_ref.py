"""Torch-CPU restatement of nucleus (top-p) filtering over the top-k survivors of a logits row, on top of
``oracle.ref_path.BeamBook.keep_top_k`` -- what ``dh_beam_row_sample_nucleus`` and ``generate_batch(..., top_p=p)`` must compute.

For one row with ``0 < top_p < 1``:

1. survivors are ``keep_top_k``'s (logits ``>=`` the ``top_k``-th largest, ties kept, ``<unk>`` dropped);
   ``p = softmax(survivors / temperature)``;
2. survivors ordered by ``p`` descending, equal ``p`` by token index ascending;
3. the survivor at sorted position ``j`` stays iff the exclusive prefix ``p[0] + ... + p[j-1]`` (fp32) is ``< top_p`` or
   ``j < beam_size``;
4. ``beam_size`` winners of ``p / Exp(1)`` among those that stay (``p`` NOT renormalised: a common factor does not change the
   race), values = ``log_softmax`` over the picks' untempered logits.

The *margin* of a row is the smallest ``|exclusive prefix - top_p|`` over its survivors: a nucleus boundary closer than the
fp32 disagreement of two summation orders (~1e-6) or of two logits computations (~1e-3 of a logit) is a coin toss, so tests
assert a margin on their INPUTS before they compare anything."""
import contextlib

import torch


def nucleus_keep(filtered, temperature, top_p, beam_size):
    """``filtered [rows, V]`` fp32 with ``-inf`` at every dropped column (``keep_top_k``'s result) -> ``(keep bool [rows, V],
    margin float)``: steps 1-3 and the smallest ``|exclusive prefix - top_p|`` met at any survivor of any row."""
    surv = torch.isfinite(filtered)
    p = torch.softmax(filtered.float() / temperature, dim=-1)
    key = torch.where(surv, p, torch.full_like(p, -1.0))                 # dropped columns sort behind every survivor
    order = torch.sort(key, dim=-1, descending=True, stable=True).indices   # stable: equal p keeps the lower index first
    ps = torch.gather(p, 1, order)
    ss = torch.gather(surv, 1, order)
    ps = torch.where(ss, ps, torch.zeros_like(ps))
    # exclusive prefix, added left to right in fp32 (torch.cumsum accumulates a float row in double); survivors come first
    excl = torch.full_like(ps, 2.0)
    run = torch.zeros_like(ps[:, 0])
    for j in range(int(ss.sum(-1).max())):
        excl[:, j] = run
        run = run + ps[:, j]
    pos = torch.arange(filtered.shape[1])[None, :]
    keep_sorted = ss & ((excl < top_p) | (pos < beam_size))
    keep = torch.zeros_like(surv)
    keep.scatter_(1, order, keep_sorted)
    gap = (excl - top_p).abs()[ss]
    margin = float(gap.min()) if gap.numel() else float("inf")
    return keep, margin


def nucleus_filter_(filtered, temperature, top_p, beam_size):
    """Step 3 as an IN-PLACE ``-inf`` mask on ``keep_top_k``'s result; returns ``(filtered, margin)``."""
    keep, margin = nucleus_keep(filtered, temperature, top_p, beam_size)
    filtered[~keep] = float("-inf")
    return filtered, margin


def nucleus_row_sample(logits, noise, temperature, beam_size, top_k, top_p, unk_index=1):
    """Steps 1-4 for ``logits [rows, V]`` with supplied Exp(1) ``noise [rows, V]`` -> ``(picks int64 [rows, beam], values fp32
    [rows, beam], margin, keep bool [rows, V])``."""
    from oracle.ref_path import BeamBook
    book = BeamBook(temperature, beam_size, top_k, unk_index=unk_index)
    filt = book.keep_top_k(logits.clone().float())
    p = torch.softmax(filt / temperature, dim=-1)
    keep, margin = nucleus_keep(filt, temperature, top_p, beam_size)
    q = torch.where(keep, p / noise, torch.full_like(p, -1.0))
    picks = torch.topk(q, beam_size, dim=-1).indices
    values = torch.gather(filt, 1, picks).log_softmax(-1)
    return picks, values, margin, keep


@contextlib.contextmanager
def patched_keep_top_k(top_p, record=None):
    """Inside the block ``oracle.ref_path.BeamBook.keep_top_k`` appends step 3 (in-place ``-inf`` mask) to its result, so that the
    model-level oracles (``ref_path.model_generate``) sample from the nucleus; the file is left alone.  ``record``: a list that
    receives every call's margin."""
    from oracle import ref_path as R
    orig = R.BeamBook.keep_top_k

    def keep_top_k(book, logits):
        out = orig(book, logits)
        _, margin = nucleus_filter_(out, book.t, top_p, book.b)
        if record is not None:
            record.append(margin)
        return out
    R.BeamBook.keep_top_k = keep_top_k
    try:
        yield
    finally:
        R.BeamBook.keep_top_k = orig
