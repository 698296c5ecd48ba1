"""``return_logprobs`` restated on torch-CPU tensors.

``pick_logprobs`` / ``record`` / ``gather`` mirror the three launches of ``csrc/beam_logprobs.hip`` (``dh_beam_pick_logprobs``,
``dh_beam_record_logprobs``, ``dh_beam_gather_logprobs``) statement for statement; ``record`` and ``gather`` only move values, so on the
kernels' own inputs they are exact in any type.  ``track`` is a second statement of the whole feature that shares no code with the
slab tables: it follows the engine's snapshots forwards, one fp64 row per beam, copying parent rows the way the select copies token
rows, and reads every value off the logits with ``log_softmax`` at the token the row received -- no picks, no back-pointers."""
import torch


def pick_logprobs(logits, pick_idx, ended, temperature):
    """fp64 ``[rows, beam]``: ``log_softmax(logits / T)`` at every row's picks; zeros for a row whose ``ended`` flag (one per logits
    row) is set or that holds nothing finite."""
    x = logits.double() / float(temperature)
    lse = torch.logsumexp(x, -1, keepdim=True)
    out = x.gather(1, pick_idx.long()) - lse
    dead = torch.as_tensor(ended).bool() | ~torch.isfinite(lse[:, 0])
    out[dead] = 0.0
    return out


def record(lp_w, par_w, step_index, tokens, parent, done, end_step, pick_idx, pick_lp, beam, first, write_pos, first_pos=None):
    """Launch 2 in place on ``lp_w`` / ``par_w`` ``[n_pos, rows]``: slab ``step_index``."""
    rows = par_w.shape[1]
    for row in range(rows):
        img = row // beam
        is_first = bool(first)
        if first_pos is not None:
            fp = int(first_pos[img])
            if step_index < fp:
                continue
            is_first = step_index == fp
        if int(done[img]) and int(end_step[img]) < step_index:
            continue
        par = int(parent[row])
        par_w[step_index, row] = par
        if write_pos >= tokens.shape[1]:
            continue
        prow = (img * beam if first_pos is not None else img) if is_first else par
        tok = int(tokens[row, write_pos])
        val = 0.0
        for j in range(beam):
            if int(pick_idx[prow, j]) == tok:
                val = pick_lp[prow, j]
                break
        lp_w[step_index, row] = val


def gather(lp_w, par_w, index, lengths, width, pos=0, first_pos=None):
    """Launch 3: ``[n, beam, width]`` in ``lp_w``'s type."""
    n, beam = index.shape
    n_pos = lp_w.shape[0]
    out = torch.zeros((n, beam, width), dtype=lp_w.dtype)
    for i in range(n):
        p0 = int(first_pos[i]) if first_pos is not None else pos
        for j in range(beam):
            r = i * beam + int(index[i, j])
            for c in range(n_pos - 1, -1, -1):
                if c < width and p0 <= c < int(lengths[i, j]):
                    out[i, j, c] = lp_w[c, r]
                r = int(par_w[c, r])
    return out


def new_tables(n_pos, rows, dtype=torch.float64):
    """What the helper fills once per session: zeros, and every row's own index."""
    return torch.zeros((n_pos, rows), dtype=dtype), torch.arange(rows, dtype=torch.int32).repeat(n_pos, 1)


def track(steps, final):
    """fp64 ``[n, beam, width]`` from the snapshot records of a whole call.  ``steps``: per beam step a dict with ``logits`` (fp32, as
    the row step saw them), ``before`` / ``after`` (the engine's state: ``tokens``, ``ended``, ``done``, ``parent``), ``first``,
    ``write_pos``, ``step``, ``first_pos`` (a list for a prompted step, else ``None``), ``temperature``, ``beam`` and ``skipped`` (the
    step made no launch).  ``final``: ``beam_index`` / ``lengths`` ``[n, beam]``, ``pos``, ``first_pos`` (list or ``None``), ``width``."""
    width = final["width"]
    n, b = final["beam_index"].shape
    cur = torch.zeros((n * b, width), dtype=torch.float64)
    for rec in steps:
        if rec.get("skipped"):
            continue
        assert rec["beam"] == b
        logp = torch.log_softmax(rec["logits"].double() / rec["temperature"], -1)
        before, after, wp = rec["before"], rec["after"], rec["write_pos"]
        new = cur.clone()
        for img in range(n):
            first = bool(rec["first"])
            if rec["first_pos"] is not None:
                if rec["step"] < rec["first_pos"][img]:
                    continue                                          # still forced: nothing was drawn
                first = rec["step"] == rec["first_pos"][img]
            if int(before["done"][img]):
                continue                                              # frozen since an earlier step
            for row in range(img * b, (img + 1) * b):
                par = int(after["parent"][row])
                new[row] = cur[par]
                if wp >= width:
                    continue
                if first:                                             # one row of logits per image: compact (dense) or the base row
                    lrow = img if logp.shape[0] == n else img * b
                    value = logp[lrow, int(after["tokens"][row, wp])]
                elif int(before["ended"][par]):
                    value = 0.0                                       # an ended beam's one candidate adds nothing
                else:
                    value = logp[par, int(after["tokens"][row, wp])]
                new[row, wp] = value
        cur = new
    out = torch.zeros((n, b, width), dtype=torch.float64)
    for i in range(n):
        p0 = final["first_pos"][i] if final["first_pos"] is not None else final["pos"]
        for j in range(b):
            row = cur[i * b + int(final["beam_index"][i, j])]
            hi = int(final["lengths"][i, j])
            out[i, j, p0:hi] = row[p0:hi]
    return out
