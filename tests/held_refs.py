"""fp64 references of the constrained draws (no GPU, no library): what mst_frame_step_held and mst_token_step_held must write, given
the stored 16-bit logits (as fp64) and — for the free cells, whose draw is mst_frame_step's own and is tested there — the frames
of the unconstrained launch on the same inputs."""
import numpy as np

FLOOR = 1e-30  # the launches' floor under a probability before the logarithm


def frame_costs(logits, tau=1.0):
    """-> (-log max(p, FLOOR), -log max(1 - p, FLOOR)) per cell, p = sigmoid(logit / tau); p and 1 - p each from their own
    exponential, as the kernel forms them (1 - p keeps its digits for a large logit)"""
    x = np.asarray(logits, np.float64) / float(tau)
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-x))
        q = 1.0 / (1.0 + np.exp(x))
    return -np.log(np.maximum(p, FLOOR)), -np.log(np.maximum(q, FLOOR))


def frame_step_held(logits, given, hold, free_frames, tau=1.0):
    """logits [N, P] fp64; given, hold [N, P] (any integer type, non-zero = set); free_frames [N, P]: the unconstrained launch's
    frames. -> (frames uint8 [N, P], free cost [N], held cost [N]): a held cell is given != 0 and is charged to the held sum, a
    free cell is the unconstrained frame and is charged to the free sum"""
    held = np.asarray(hold) != 0
    frames = np.where(held, np.asarray(given) != 0, np.asarray(free_frames) != 0)
    on, off = frame_costs(logits, tau)
    cost = np.where(frames, on, off)
    return frames.astype(np.uint8), np.where(held, 0.0, cost).sum(1), np.where(held, cost, 0.0).sum(1)


def token_cost(logits, token):
    """-log max(softmax(logits)[token], FLOOR) of one row (fp64): the model's own distribution, temperature 1, uncut"""
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max())
    return -np.log(max(e[int(token)] / e.sum(), FLOOR))


def token_step_held(logits, given, hold, finished, free_tokens, eos, pad):
    """one position for N sequences. logits [N, V] fp64; given [N] tokens; hold [N]; finished [N] bool (the sequence had ended
    before this position); free_tokens [N]: the unconstrained launch's tokens. -> (tokens [N], held cost [N], running [int]):
    a held position writes given (PAD if it is outside [0, V)) whatever the state and is charged unless finished"""
    logits = np.asarray(logits, np.float64)
    N, V = logits.shape
    tokens, cost = np.zeros(N, np.int64), np.zeros(N)
    for n in range(N):
        if hold[n]:
            ok = 0 <= int(given[n]) < V
            tokens[n] = int(given[n]) if ok else pad
            if ok and not finished[n]:
                cost[n] = token_cost(logits[n], given[n])
        else:
            tokens[n] = free_tokens[n]
    return tokens, cost, int(((tokens != eos) & (tokens != pad)).sum())
