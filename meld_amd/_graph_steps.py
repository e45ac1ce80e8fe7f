"""What the steps over a fitted graph's CSR arrays share on the host side (``components``, ``diffuse``, ``geodesic``): the
unsharded-graph rule, the operands of a matrix without entries, and the loop that repeats a round until it changes nothing."""
from __future__ import annotations


def is_sharded(G):
    return G.n_rows != G.N or getattr(G, "comm", None) is not None


def require_unsharded(G, what):
    """ValueError ``"<what> only defined for an unsharded graph"`` on a row shard."""
    if is_sharded(G):
        raise ValueError("{} only defined for an unsharded graph".format(what))


def csr_operands(G, values):
    """``(rowptr, col, values)`` for a C entry that streams the graph's entries with ``values`` next to ``G.col``; a matrix without
    entries gets one-element placeholders (any address serves, none is read)."""
    import torch

    if G.nnz == 0:
        dev = G.rowptr.device
        return G.rowptr, torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    return G.rowptr, G.col, values


def rounds_until_unchanged(step, changed, max_rounds, describe):
    """Call ``step(round)`` for round 0, 1, ... until one leaves the device word ``changed`` at 0 (the one word the host reads
    per round); the number of rounds, that idle one included.  RuntimeError ``describe(rounds)`` when ``max_rounds`` rounds
    have not got there."""
    rounds = 0
    while True:
        if rounds >= max_rounds:
            raise RuntimeError(describe(rounds))
        step(rounds)
        rounds += 1
        if int(changed.item()) == 0:
            return rounds
