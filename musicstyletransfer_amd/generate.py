"""Generation from the latent space: draws from the prior, posterior draws at a temperature, interpolation between two melodies,
style transfer from ONE encode, and blends of two class embeddings.

A request is a RECIPE — per output row which source vectors to mix (a, b, w), how much noise to add (tau, optionally scaled by the
encoder's sigma) and which class embeddings to mix (ca, cb, cw) — built on the host by the functions below (pure numpy: they are what
the CPU tests check), turned into latent vectors and decoder start rows by ONE launch per chunk (ops.latent_rows: mst_latent_rows),
and decoded by what the samplers use: decode.AncestralSampling / decode.BeamSearch for the token ends (decode.TokenSampling when the
draw has a temperature, a top-k or a nucleus cut), decode.FrameSampling for the piano-roll ends. The reference stops at `latent_vector = means` (sampler.py:146-148); nothing here has a counterpart there.

Constrained decoding works on a piece that already exists: some cells of the output are GIVEN (a mask from hold_mask), the decoder is
fed them as if it had drawn them, and only the free cells are drawn — continue_ (hold an opening), repaint (hold any mask) and score
(hold everything: the piece's negative log-likelihood under a class). The held positions run through the same captured graph per
position as every other one (decode.FrameSampling / decode.TokenSampling with `given` and `hold`); DESIGN §15.

Index mapping of a piece (the training step's alignment of inputs and labels: decoder row k + 1 is fed input k and scored against
label k):
  * piano-roll ends: the piece is the batch's LABEL roll [B, T, P]; position k + 1 emits labels[:, k] (pianoroll.pianoroll_arrays: the
    input roll is the label roll moved down one frame behind the start row), so mask cell [b, k, j] is frame k, pitch j;
  * token ends: the piece is the token row with its EOS, [B, T + 1]; position i emits the token at index i, index 0 is SOS and is
    never held, and the EOS of a row of seq_len tokens (SOS included) sits at index seq_len.

likelihood is not generation at all: the importance-weighted bound on log p(piece | class) from K posterior draws per melody
(Model.iw_bound: engine.IWBound), the teacher-forced likelihood of the training step under K latent vectors — where score
decodes the piece under ONE z (the mean) through a graph per position. It prints one line per melody and writes no files.

    python -m music_style_transfer.VarAutoEncoder.generate --model-output DIR --mode transfer --data MIDI_DIR --out OUT_DIR
"""
import argparse
import math
import os

import numpy as np

from .ops import roundup
from .spec import positional_table

MODES = ("prior", "posterior", "interpolate", "transfer", "blend", "continue", "repaint", "score", "likelihood")
DECODERS = ("sampling", "greedy", "beam")


class Recipe:
    """N rows of mst_latent_rows' inputs, what each row is (`rows`: one dict per row) and the name of the file it is written to"""

    def __init__(self, name, a, b, w, ca, cb, cw, rows, files, tau=0.0, use_sigma=False, mode="lerp"):
        self.name = name
        self.a, self.b = np.asarray(a, np.int32).reshape(-1), np.asarray(b, np.int32).reshape(-1)
        self.ca, self.cb = np.asarray(ca, np.int32).reshape(-1), np.asarray(cb, np.int32).reshape(-1)
        self.w, self.cw = np.asarray(w, np.float32).reshape(-1), np.asarray(cw, np.float32).reshape(-1)
        self.rows, self.files = list(rows), list(files)
        self.tau, self.use_sigma, self.mode = float(tau), bool(use_sigma), mode
        n = len(self.a)
        if not all(len(x) == n for x in (self.b, self.w, self.ca, self.cb, self.cw, self.rows, self.files)):
            raise ValueError("recipe arrays differ in length")
        if mode not in ("lerp", "slerp"):
            raise ValueError("interpolation mode must be 'lerp' or 'slerp', got {!r}".format(mode))
        if self.tau < 0:
            raise ValueError("temperature must not be negative")

    def __len__(self):
        return len(self.a)

    def validate(self, n_sources, n_classes):
        """the kernel clamps indices into its tables; a recipe that would need the clamp is refused here"""
        src = np.concatenate([self.a, self.b])
        if (src >= n_sources).any() or (self.b[self.a >= 0] < 0).any():
            raise ValueError("recipe {!r} names a source row outside [0, {})".format(self.name, n_sources))
        cls = np.concatenate([self.ca, self.cb])
        if (cls < 0).any() or (cls >= n_classes).any():
            raise ValueError("recipe {!r} names a class outside [0, {})".format(self.name, n_classes))
        if not (np.isfinite(self.w).all() and np.isfinite(self.cw).all()):
            raise ValueError("recipe {!r} has a weight that is not finite".format(self.name))


def _classes(classes, n, what):
    c = np.asarray(classes, np.int64).reshape(-1)
    if c.size == 1:
        c = np.full(n, int(c[0]), np.int64)
    if c.size != n:
        raise ValueError("{}: {} classes for {} rows".format(what, c.size, n))
    return c


def recipe_prior(n, classes, temperature=1.0):
    """z ~ N(0, temperature^2 I), one class per row (one class for all rows if a single one is given)"""
    if n <= 0:
        raise ValueError("prior: n must be positive")
    c = _classes(classes, n, "prior")
    rows = [dict(n=k, cls=int(c[k])) for k in range(n)]
    files = ["prior-{}.class-{}.mid".format(k, int(c[k])) for k in range(n)]
    z = np.zeros(n)
    return Recipe("prior", z - 1, z - 1, z, c, c, z, rows, files, tau=temperature)


def recipe_posterior(batch_classes, n_per_sample, temperature=1.0):
    """z = mu + temperature * eps * sigma, n_per_sample draws of every melody (melody-major), the melody's own class"""
    c = np.asarray(batch_classes, np.int64).reshape(-1)
    if n_per_sample <= 0:
        raise ValueError("posterior: n_per_sample must be positive")
    a = np.repeat(np.arange(len(c)), n_per_sample)
    d = np.tile(np.arange(n_per_sample), len(c))
    rows = [dict(melody=int(i), draw=int(k), cls=int(c[i])) for i, k in zip(a, d)]
    files = ["posterior-{}.draw-{}.mid".format(int(i), int(k)) for i, k in zip(a, d)]
    z = np.zeros(len(a))
    return Recipe("posterior", a, a, z, c[a], c[a], z, rows, files, tau=temperature, use_sigma=True)


def recipe_interpolate(i, j, steps, class_i, class_j, classes=None, mode="slerp"):
    """`steps` points from melody i (weight 0) to melody j (weight 1), both included; the class is i's up to and including the
    middle step and j's behind it, or `classes` (one per step)"""
    if steps < 2:
        raise ValueError("interpolate: at least the two end points (steps >= 2)")
    w = np.linspace(0.0, 1.0, steps).astype(np.float32)
    if classes is None:
        c = np.where(2 * np.arange(steps) <= steps - 1, int(class_i), int(class_j))
    else:
        c = _classes(classes, steps, "interpolate")
    rows = [dict(melody_a=int(i), melody_b=int(j), step=s, weight=float(w[s]), cls=int(c[s])) for s in range(steps)]
    files = ["interp-{}-{}.{:02d}.mid".format(int(i), int(j), s) for s in range(steps)]
    z = np.zeros(steps)
    return Recipe("interpolate", z + i, z + j, w, c, c, z, rows, files, mode=mode)


def recipe_transfer(n_melodies, target_classes):
    """every melody x every target class (melody-major): z = mu of the melody, the class embedding of the target"""
    t = np.asarray(target_classes, np.int64).reshape(-1)
    if n_melodies <= 0 or t.size == 0:
        raise ValueError("transfer: no melody or no target class")
    a = np.repeat(np.arange(n_melodies), t.size)
    c = np.tile(t, n_melodies)
    rows = [dict(melody=int(i), cls=int(k)) for i, k in zip(a, c)]
    files = ["transfer-{}.class-{}.mid".format(int(i), int(k)) for i, k in zip(a, c)]
    z = np.zeros(len(a))
    return Recipe("transfer", a, a, z, c, c, z, rows, files)


def recipe_class_blend(n_melodies, class_a, class_b, weights):
    """z = mu of the melody, class embedding (1 - weight) * class_a + weight * class_b, for every melody x weight (melody-major)"""
    wts = np.asarray(weights, np.float32).reshape(-1)
    if n_melodies <= 0 or wts.size == 0:
        raise ValueError("class_blend: no melody or no weight")
    a = np.repeat(np.arange(n_melodies), wts.size)
    k = np.tile(np.arange(wts.size), n_melodies)
    rows = [dict(melody=int(i), cls_a=int(class_a), cls_b=int(class_b), step=int(s), weight=float(wts[s])) for i, s in zip(a, k)]
    files = ["blend-{}.class-{}-{}.{:02d}.mid".format(int(i), int(class_a), int(class_b), int(s)) for i, s in zip(a, k)]
    z = np.zeros(len(a))
    return Recipe("blend", a, a, z, z + class_a, z + class_b, wts[k], rows, files)


def _own_or_target(batch_classes, target_classes, what):
    c = np.asarray(batch_classes, np.int64).reshape(-1)
    return c if target_classes is None else _classes(target_classes, len(c), what)


def recipe_continue(batch_classes, n_per_sample=1, target_classes=None):
    """z = mu of the (encoded opening of the) melody, n_per_sample rows per melody (melody-major: they differ by the draw of the free
    cells), the melody's own class or target_classes (one for all, or one per melody)"""
    if n_per_sample <= 0:
        raise ValueError("continue: n_per_sample must be positive")
    c = _own_or_target(batch_classes, target_classes, "continue")
    a = np.repeat(np.arange(len(c)), n_per_sample)
    d = np.tile(np.arange(n_per_sample), len(c))
    rows = [dict(melody=int(i), draw=int(k), cls=int(c[i])) for i, k in zip(a, d)]
    files = ["continue-{}.draw-{}.mid".format(int(i), int(k)) for i, k in zip(a, d)]
    z = np.zeros(len(a))
    return Recipe("continue", a, a, z, c[a], c[a], z, rows, files)


def recipe_repaint(batch_classes, target_classes=None):
    """z = mu of the melody, one row per melody, its own class or target_classes (one for all, or one per melody)"""
    c = _own_or_target(batch_classes, target_classes, "repaint")
    a = np.arange(len(c))
    rows = [dict(melody=int(i), cls=int(c[i])) for i in a]
    files = ["repaint-{}.class-{}.mid".format(int(i), int(c[i])) for i in a]
    z = np.zeros(len(a))
    return Recipe("repaint", a, a, z, c, c, z, rows, files)


def recipe_score(n_melodies, target_classes):
    """transfer's rows (every melody x every class, melody-major) under the name 'score'"""
    r = recipe_transfer(n_melodies, target_classes)
    r.name = "score"
    r.files = ["score-{}.class-{}.mid".format(row["melody"], row["cls"]) for row in r.rows]
    return r


def hold_mask(lens, T, P=None, time=None, pitch=None):
    """the cells of a piece to hold: bool [B, T] (P None: token ends) or [B, T, P] (piano-roll ends), true inside the half-open
    `time` = (first, behind) range of the piece's time index and, for rolls, inside the half-open `pitch` range; a range that is
    omitted means everything, an empty one nothing. Never true at or behind a row's `lens`. (The piece's indexing is the module
    docstring's: frame k of the label roll; token index i of the row, where index 0 is SOS.)"""
    lens = np.asarray(lens, np.int64).reshape(-1)
    T = int(T)
    if T <= 0 or (P is not None and int(P) <= 0):
        raise ValueError("hold_mask: T and P must be positive")
    t = np.arange(T)
    m = t[None, :] < lens[:, None]
    if time is not None:
        lo, hi = (int(v) for v in time)
        m = m & ((t >= lo) & (t < hi))[None, :]
    if P is None:
        if pitch is not None:
            raise ValueError("hold_mask: a pitch range needs P (piano-roll ends)")
        return m
    j = np.arange(int(P))
    pm = np.ones(int(P), bool)
    if pitch is not None:
        lo, hi = (int(v) for v in pitch)
        pm = (j >= lo) & (j < hi)
    return m[:, :, None] & pm[None, None, :]


def token_piece(tokens, seq_lens):
    """token rows [B, T] (SOS first, PAD behind seq_len) -> the piece [B, T + 1] with EOS at index seq_len"""
    from .MIDIUtil.defaults import EOS_ID, PAD_ID
    tokens, lens = np.asarray(tokens, np.int64), np.asarray(seq_lens, np.int64).reshape(-1)
    B, T = tokens.shape
    piece = np.full((B, T + 1), PAD_ID, np.int64)
    piece[:, :T] = np.where(np.arange(T)[None, :] < lens[:, None], tokens, PAD_ID)
    piece[np.arange(B), np.clip(lens, 0, T)] = EOS_ID
    return piece


def opening(tokens, seq_lens, prime):
    """what continue_ encodes: the input with everything behind the first `prime` rows zeroed, and seq_lens clipped to prime"""
    prime = int(prime)
    if prime < 1:
        raise ValueError("continue: prime must be at least 1")
    x = np.array(tokens, copy=True)
    x[:, prime:] = 0
    return x, np.minimum(np.asarray(seq_lens, np.int64).reshape(-1), prime)


def chunks(n_rows, max_rows):
    """[lo, hi) ranges of at most max_rows rows; the noise of row r is a function of r, so the chunking does not change it"""
    if max_rows <= 0:
        raise ValueError("max_rows must be positive")
    return [(lo, min(lo + max_rows, n_rows)) for lo in range(0, n_rows, max_rows)]


def ids_to_melody(ids):
    """token row -> Melody: PAD / SOS dropped, cut at the first EOS (what the samplers write)"""
    from .MIDIUtil.defaults import EOS_ID, PAD_ID, SOS_ID
    from .MIDIUtil.Melody import get_melody_from_ids
    ids = [int(i) for i in np.asarray(ids).reshape(-1) if int(i) not in (PAD_ID, SOS_ID)]
    if EOS_ID in ids:
        ids = ids[: ids.index(EOS_ID)]
    return get_melody_from_ids(np.asarray(ids, np.int64))


class Generated:
    """what a LatentGenerator call returns: `z` (host fp32 [N, Z]), `rows` (what every row is), `sequences` (token ids [N, L], token
    ends) or `rolls` (uint8 [N, frames, P], piano-roll ends), `scores` (summed -log p of what was decoded), `start_rows` (the decoder
    rows of position 0, host copy in the activation type), `probs` (piano-roll ends with keep_probs: fp32 [N, frames, P]); of a
    constrained call also `hold` (bool, the mask of every row in the piece's indexing) and `held_scores` (fp64 [N]: the summed
    -log p of the held cells, which `scores` then does not contain)"""

    def __init__(self, recipe, z, start_rows, scores, sequences=None, rolls=None, probs=None, slices_per_quarter=4, held_scores=None,
                 hold=None):
        self.name, self.rows, self.files = recipe.name, recipe.rows, recipe.files
        self.z, self.start_rows, self.scores = z, start_rows, scores
        self.held_scores, self.hold = held_scores, hold
        self.sequences, self.rolls, self.probs = sequences, rolls, probs
        self.slices_per_quarter = slices_per_quarter

    def __len__(self):
        return len(self.rows)

    def melodies(self):
        if self.sequences is not None:
            return [ids_to_melody(s) for s in self.sequences]
        from .pianoroll import pianoroll_to_melody
        return [pianoroll_to_melody(r, self.slices_per_quarter) for r in self.rolls]

    def write(self, folder, names=None):
        """one .mid per row into `folder` (names: the recipe's, e.g. transfer-0.class-1.mid); returns the paths"""
        from .MIDIUtil.midi_io import MelodyWriter
        os.makedirs(folder, exist_ok=True)
        writer, out = MelodyWriter(), []
        for name, melody in zip(names or self.files, self.melodies()):
            out.append(os.path.join(folder, name))
            writer.write_to_file(out[-1], melody)
        return out


class LatentGenerator:
    """model: an initialised VarAutoEncoder.model.Model. decoder: 'sampling' (ancestral draws), 'greedy' (the most likely token /
    every pitch above one half) or 'beam' (token ends only). temperature: the scale of the latent noise (prior and posterior draws).
    sample_temperature, top_k, top_p: the DRAW's own settings (decoder 'sampling'): logits are divided by sample_temperature; the token
    ends keep the top_k most likely tokens (0: all) and of those the smallest set reaching top_p (1: all) — decode.TokenSampling; with
    all three at their defaults the token ends draw from the raw softmax (decode.AncestralSampling). frame_temperature: the piano-roll
    ends' earlier name of sample_temperature. More than max_rows rows are decoded in chunks."""

    def __init__(self, model, attention=None, seed=0, temperature=1.0, decoder="sampling", beam_size=4, max_rows=256,
                 frame_temperature=1.0, keep_probs=False, sample_temperature=1.0, top_k=0, top_p=1.0):
        if decoder not in DECODERS:
            raise ValueError("decoder must be one of {}, got {!r}".format(DECODERS, decoder))
        if max_rows <= 0:
            raise ValueError("max_rows must be positive")
        sample_temperature, top_k, top_p = float(sample_temperature), int(top_k), float(top_p)
        if not 0.0 < sample_temperature < float("inf") or top_k < 0 or not 0.0 < top_p <= 1.0:
            raise ValueError("sample_temperature > 0, top_k >= 0 and 0 < top_p <= 1 wanted, got {}, {}, {}".format(sample_temperature, top_k, top_p))
        if (top_k != 0 or top_p != 1.0) and decoder != "sampling":
            raise ValueError("top_k and top_p cut the distribution that decoder 'sampling' draws from; decoder {!r} draws nothing".format(decoder))
        if (top_k != 0 or top_p != 1.0) and model is not None and model.engine_config.kind != "token":
            raise ValueError("top_k and top_p rank tokens; a piano-roll frame is one Bernoulli draw per pitch (sample_temperature applies)")
        if sample_temperature != 1.0 and float(frame_temperature) != 1.0 and sample_temperature != float(frame_temperature):
            raise ValueError("frame_temperature is the earlier name of sample_temperature: give one of them")
        self.sample_temperature, self.top_k, self.top_p = sample_temperature, top_k, top_p
        self.last_sampler = None  # the decode.* object of the latest chunk
        self.model, self._attention, self.seed = model, attention, int(seed)
        self.temperature, self.decoder, self.beam_size, self.max_rows = float(temperature), decoder, int(beam_size), int(max_rows)
        self.frame_temperature = sample_temperature if sample_temperature != 1.0 else float(frame_temperature)
        self.keep_probs = bool(keep_probs)
        self.calls = 0
        self._samplers, self._pos0 = {}, None
        if model is not None and decoder == "beam" and model.engine_config.kind != "token":
            raise ValueError("beam search ranks token sequences; the piano-roll ends decode with 'sampling' or 'greedy'")

    # ------------------------------------------------------------------ the modes
    def encode(self, batch):
        """(mu, sigma) of a batch (device fp32 [B, Z]): the encoder and the latent launch only (Model.encode)"""
        tokens, seq_lens, classes = batch.data[:3]
        return self.model.encode(tokens, seq_lens, classes)

    def prior(self, n, classes, length):
        return self._run(recipe_prior(n, classes, self.temperature), None, None, length)

    def posterior(self, batch, n_per_sample, length=None):
        mu, sigma = self.encode(batch)
        return self._run(recipe_posterior(batch.data[2], n_per_sample, self.temperature), mu, sigma, self._length(batch, length))

    def interpolate(self, batch, i, j, steps, mode="slerp", classes=None, length=None):
        cls = np.asarray(batch.data[2]).reshape(-1)
        mu, _ = self.encode(batch)
        return self._run(recipe_interpolate(i, j, steps, cls[i], cls[j], classes, mode), mu, None, self._length(batch, length))

    def transfer(self, batch, target_classes=None, length=None):
        """every melody of the batch in every target class (default: all of the model's) from ONE encode"""
        if target_classes is None:
            target_classes = np.arange(self.model.engine_config.num_classes)
        mu, _ = self.encode(batch)
        return self._run(recipe_transfer(len(np.asarray(batch.data[2])), target_classes), mu, None, self._length(batch, length))

    def class_blend(self, batch, class_a, class_b, weights, length=None):
        mu, _ = self.encode(batch)
        return self._run(recipe_class_blend(len(np.asarray(batch.data[2])), class_a, class_b, weights), mu, None,
                         self._length(batch, length))

    # ------------------------------------------------------------------ constrained decoding (module docstring: the index mapping)
    def _constrainable(self):
        if self.decoder == "beam":
            raise ValueError("beam search takes no constraints: decode a constrained piece with 'sampling' or 'greedy'")

    def _piece(self, batch):
        """-> (piece, lens, is_token): the label roll [B, T, P] with the rows' lengths, or the token rows with their EOS [B, T + 1] and
        lens = the index behind the EOS"""
        tokens, seq_lens = np.asarray(batch.data[0]), np.asarray(batch.data[1], np.int64).reshape(-1)
        if tokens.ndim == 2:
            return token_piece(tokens, seq_lens), seq_lens + 1, True
        if not batch.label:
            raise ValueError("a piano-roll piece is the batch's label roll: the batch has no label")
        return (np.asarray(batch.label[0]) != 0).astype(np.uint8), seq_lens, False

    def _constrained(self, recipe, mu, piece, hold, length):
        piece, hold = np.asarray(piece), np.asarray(hold) != 0
        if hold.shape[0] != piece.shape[0] or hold.ndim != piece.ndim or hold.shape[2:] != piece.shape[2:] or hold.shape[1] > piece.shape[1]:
            raise ValueError("the mask {} does not fit the piece {}".format(hold.shape, piece.shape))
        full = np.zeros(piece.shape, bool)
        full[:, : hold.shape[1]] = hold
        n = min(piece.shape[1], length - 1 if piece.ndim == 3 else length)  # a shorter run cuts the piece
        return self._run(recipe, mu, None, length, given=piece[recipe.a, :n], hold=full[recipe.a, :n])

    def continue_(self, batch, prime, n_per_sample=1, target_classes=None, length=None):
        """continue an opening: the first `prime` frames (or tokens behind SOS) of every melody are held — for the token ends never at or
        behind the opening's EOS — and the rest is drawn, n_per_sample times per melody. The latent vector is that of the OPENING ONLY:
        the encoder sees the input with seq_lens clipped to prime and everything behind zeroed. target_classes restyles the continuation."""
        self._constrainable()
        tokens, seq_lens, classes = batch.data[:3]
        recipe = recipe_continue(classes, n_per_sample, target_classes)
        x, lens = opening(tokens, seq_lens, prime)
        piece, piece_lens, token = self._piece(batch)
        if token:  # indices 1 .. prime, short of the EOS at index piece_lens - 1
            hold = hold_mask(piece_lens - 1, piece.shape[1], time=(1, int(prime) + 1))
        else:
            hold = hold_mask(piece_lens, piece.shape[1], piece.shape[2], time=(0, int(prime)))
        mu, _ = self.model.encode(x, lens, classes)
        return self._constrained(recipe, mu, piece, hold, self._length(batch, length))

    def repaint(self, batch, hold, target_classes=None, length=None):
        """keep the cells of `hold` (hold_mask: [B, T, P] over the label roll, or [B, <= T + 1] over the token row) and redraw the others;
        the whole piece is encoded"""
        self._constrainable()
        recipe = recipe_repaint(batch.data[2], target_classes)
        piece, _, _ = self._piece(batch)
        mu, _ = self.encode(batch)
        return self._constrained(recipe, mu, piece, hold, self._length(batch, length))

    def score(self, batch, target_classes=None):
        """how well does class c explain this piece: everything up to each row's length is held, for every (melody, class) pair in
        transfer's order; held_scores[r] of the result is the piece's negative log-likelihood under that class. ONE encode."""
        self._constrainable()
        if target_classes is None:
            target_classes = np.arange(self.model.engine_config.num_classes)
        recipe = recipe_score(len(np.asarray(batch.data[2]).reshape(-1)), target_classes)
        piece, lens, token = self._piece(batch)
        hold = hold_mask(lens, piece.shape[1], time=(1, piece.shape[1])) if token else hold_mask(lens, piece.shape[1], piece.shape[2])
        mu, _ = self.encode(batch)
        return self._constrained(recipe, mu, piece, hold, piece.shape[1] if token else piece.shape[1] + 1)

    # ------------------------------------------------------------------ recipe -> rows -> decoded pieces
    @staticmethod
    def _length(batch, length):
        return int(length) if length is not None else 2 * np.asarray(batch.data[0]).shape[1]  # (sampler.py:163)

    def _decode(self, row0, length, seed, given=None, hold=None):
        """-> (sequences or rolls, scores, probs, held_scores) of one chunk as host arrays; given, hold: the chunk's rows of a
        constrained call (held_scores is None without them)"""
        if given is not None:
            self._constrainable()
        from . import decode
        from .VarAutoEncoder.model import resolve_attention
        m, n = self.model, row0.shape[0]
        attention = resolve_attention(m.engine_config, self._attention)
        if m.engine_config.kind != "token":
            if self.top_k != 0 or self.top_p != 1.0:
                raise ValueError("top_k and top_p rank tokens; a piano-roll frame is one Bernoulli draw per pitch")
            fs = self.last_sampler = m.frame_sampling_plan(n, length, attention, keep_probs=self.keep_probs)
            roll, scores = fs.run(row0, length, tau=self.frame_temperature, mode="draw" if self.decoder == "sampling" else "threshold",
                                  thr=0.5, seed=seed, given=given, hold=hold)
            return (roll, scores, (fs.probs[:, : length - 1].cpu().numpy() if self.keep_probs else None),
                    fs.held_scores if given is not None else None)
        from .MIDIUtil.defaults import PAD_ID

        def padded(got):  # the rows a run returned (it may have stopped early), PAD up to `length`
            seqs = np.full((n, length), PAD_ID, np.int64)
            seqs[:, : got.shape[1]] = got
            return seqs

        if given is not None or (self.decoder == "sampling" and (self.sample_temperature != 1.0 or self.top_k != 0 or self.top_p != 1.0)):
            # (a constrained piece always decodes here; 'greedy' is then the draw among the single most likely token)
            greedy = self.decoder != "sampling"
            ts = self.last_sampler = m.token_sampling_plan(n, length, attention)
            got, scores = ts.run(row0, length, tau=1.0 if greedy else self.sample_temperature, top_k=1 if greedy else self.top_k,
                                 top_p=1.0 if greedy else self.top_p, seed=seed, given=given, hold=hold)
            return padded(got), scores, None, (ts.held_scores if given is not None else None)
        if self.decoder == "sampling":
            key = (n, length, attention, id(m.store))
            smp = self._samplers.get(key)
            if smp is None:
                if len(self._samplers) >= 4:
                    self._samplers.pop(next(iter(self._samplers)))
                smp = self._samplers[key] = decode.AncestralSampling(m.store, n, length, attention, seed=seed)
            self.last_sampler = smp
            got, scores = smp.run(row0)
            return padded(got), scores, None, None
        K = self.beam_size if self.decoder == "beam" else 1  # (one beam is greedy decoding)
        bs = self.last_sampler = m.beam_search_plan(n, K, length, attention)
        seqs, scores = bs.run(row0.repeat_interleave(K, dim=0).contiguous() if K > 1 else row0)
        return seqs.astype(np.int64).reshape(n, K, -1)[:, 0], scores.reshape(n, K)[:, 0], None, None

    def _rows(self, recipe, mu, ssrc, lo, hi, seed=0):
        """rows [lo, hi) of a recipe through mst_latent_rows -> (z fp32 [n, Z], decoder start rows [n, >= Dd]) on the device"""
        import torch
        from . import ops as o
        st, cfg = self.model.store, self.model.engine_config
        dev, Dd, n = st.device, cfg.d_model, hi - lo
        if self._pos0 is None or self._pos0.device != dev:
            self._pos0 = torch.from_numpy(np.ascontiguousarray(positional_table(Dd, 1)[:1])).to(dev)
        up = lambda x: torch.from_numpy(np.ascontiguousarray(x[lo:hi])).to(dev)
        z_out = torch.empty(n, cfg.latent_dim, dtype=torch.float32, device=dev)
        row0 = torch.zeros(n, roundup(Dd, 8), dtype=st.act_dtype, device=dev)
        o.latent_rows(mu, ssrc, up(recipe.a), up(recipe.b), up(recipe.w), up(recipe.ca), up(recipe.cb), up(recipe.cw),
                      st.p("decoder.latent2hid.weight"), st.p("decoder.latent2hid.bias"), st.p("decoder.class2hid.weight"), self._pos0,
                      math.sqrt(float(Dd)), z_out, row0, mode=recipe.mode, tau=recipe.tau, seed=seed, row0=lo)
        return z_out, row0

    def _run(self, recipe, mu, sigma, length, given=None, hold=None):
        """given, hold: one row per recipe row (constrained calls); every chunk is handed its own rows"""
        import torch
        cfg = self.model.engine_config
        recipe.validate(0 if mu is None else mu.shape[0], cfg.num_classes)
        if length < 2:
            raise ValueError("length must be at least 2 positions")
        self.calls += 1
        seed = (self.seed * 0x9E3779B97F4A7C15 + self.calls) & 0xFFFFFFFFFFFFFFFF
        zs, rows, outs, scores, probs, held = [], [], [], [], [], []
        for lo, hi in chunks(len(recipe), self.max_rows):
            z_out, row0 = self._rows(recipe, mu, sigma if recipe.use_sigma else None, lo, hi, seed)
            out, sc, pr, hs = self._decode(row0, length, seed ^ (lo * 0xD1B54A32D192ED03 & 0xFFFFFFFFFFFFFFFF),
                                           None if given is None else given[lo:hi], None if given is None else hold[lo:hi])
            held.append(None if hs is None else np.asarray(hs, np.float64))
            zs.append(z_out.cpu().numpy())
            rows.append(row0[:, : cfg.d_model].cpu())
            outs.append(out)
            scores.append(np.asarray(sc, np.float64))
            probs.append(pr)
        token = cfg.kind == "token"
        return Generated(recipe, np.concatenate(zs), torch.cat(rows), np.concatenate(scores),
                         sequences=np.concatenate(outs) if token else None, rolls=None if token else np.concatenate(outs),
                         probs=np.concatenate(probs) if probs[0] is not None else None,
                         held_scores=np.concatenate(held) if given is not None else None, hold=hold)


def likelihood_lines(model, batch, samples):
    """--mode likelihood: one line per melody of the batch — the importance-weighted bound on -log p (nats), the same draws' ELBO, the
    effective sample size of the weights, bits per cell, and whether every draw was finite"""
    if not batch.label:
        raise ValueError("the likelihood of a piece is that of the batch's labels: the batch has no label")
    tokens, seq_lens, classes = batch.data[:3]
    res = model.iw_bound(tokens, seq_lens, classes, batch.label[0], samples=samples)
    per_cell = res["cells"] * math.log(2.0)
    return ["melody {} class {} nll {:.6f} elbo_nll {:.6f} ess {:.3f} bits_per_cell {:.6f} valid {}".format(
        i, int(c), -res["log_px"][i], -res["elbo"][i], res["ess"][i], -res["log_px"][i] / per_cell, int(res["valid"][i]))
        for i, c in enumerate(np.asarray(classes).reshape(-1))]


# ---------------------------------------------------------------------- command line
def build_parser():
    p = argparse.ArgumentParser(prog="python -m music_style_transfer.VarAutoEncoder.generate",
                                description="Generate .mid files from the latent space of a trained model.")
    p.add_argument("--model-output", required=True, help="the model folder of the training run (config + params.N)")
    p.add_argument("--checkpoint", type=int, default=-1, help="checkpoint index (-1: the latest)")
    p.add_argument("--ema", action="store_true", help="decode with the checkpoint's averaged weights (a run trained with --ema-decay)")
    p.add_argument("--mode", required=True, choices=MODES)
    src = p.add_mutually_exclusive_group()
    src.add_argument("--data", default=None, help="MIDI folder (one sub-folder per class); the first batch is used")
    src.add_argument("--toy", action="store_true", help="the three toy sequences instead of --data")
    p.add_argument("--out", default=None, help="folder the .mid files are written to (every mode but score and likelihood, which print)")
    p.add_argument("--iw-samples", type=int, default=16, metavar="K",
                   help="likelihood: posterior draws per melody of the importance-weighted bound (>= 1; 1 is the one-sample ELBO)")
    p.add_argument("--n", type=int, default=4, help="prior: number of pieces; posterior: draws per melody; continue: continuations per melody")
    p.add_argument("--prime", type=int, default=None, metavar="N", help="continue: hold the first N frames / tokens of every melody")
    p.add_argument("--keep-time", type=int, nargs=2, default=None, metavar=("A", "B"),
                   help="repaint: keep frames (token indices) A <= t < B and redraw the others (default: all of them)")
    p.add_argument("--keep-pitch", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                   help="repaint, piano-roll models: keep pitches LO <= j < HI (with --keep-time: cells inside both ranges)")
    p.add_argument("--steps", type=int, default=8, help="interpolate / blend: number of points, end points included")
    p.add_argument("--pair", type=int, nargs=2, default=(0, 1), metavar=("I", "J"), help="interpolate: the two melodies of the batch")
    p.add_argument("--classes", type=int, nargs="*", default=None, help="prior / transfer: classes (default: all); blend: the two to mix")
    p.add_argument("--interpolation", default="slerp", choices=("slerp", "lerp"))
    p.add_argument("--temperature", type=float, default=1.0)
    p.add_argument("--decoder", default="sampling", choices=DECODERS)
    p.add_argument("--sample-temperature", type=float, default=1.0, help="--decoder sampling: the draw's temperature (logits are divided by it)")
    p.add_argument("--top-k", type=int, default=0, help="--decoder sampling, token models: draw among the k most likely tokens (0: all)")
    p.add_argument("--top-p", type=float, default=1.0, help="--decoder sampling, token models: ... and of those the smallest set reaching this mass (1: all)")
    p.add_argument("--beam-size", type=int, default=4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--length", type=int, default=None, help="positions to decode (default: twice the input length; prior: 2 * --max-seq-len)")
    p.add_argument("--batch-size", type=int, default=8)
    p.add_argument("--max-seq-len", type=int, default=64)
    p.add_argument("--slices-per-quarter-note", type=int, default=4)
    p.add_argument("--max-rows", type=int, default=256)
    p.add_argument("--device", type=int, default=0, help="index of the HIP device")
    return p


def _first_batch(args, kind):
    from .VarAutoEncoder.data import Loader, ToyData, load_dataset
    if args.toy:
        return next(iter(ToyData()))
    if args.data is None:
        raise SystemExit("--mode {} needs --data DIR or --toy".format(args.mode))
    loader = Loader(path=args.data, max_sequence_length=args.max_seq_len, slices_per_quarter_note=args.slices_per_quarter_note)
    kw = {}
    if kind != "token":
        from .pianoroll import PianoRollDataset
        kw = dict(dataset_cls=lambda bs, L, mel, **k: PianoRollDataset(bs, L, mel, slices_per_quarter=args.slices_per_quarter_note))
    train, _ = load_dataset(loader, args.batch_size, None, None, **kw)
    return next(iter(train))


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.mode not in ("score", "likelihood") and args.out is None:
        raise SystemExit("--mode {} needs --out DIR".format(args.mode))
    if args.mode == "continue" and args.prime is None:
        raise SystemExit("--mode continue needs --prime N")
    from .VarAutoEncoder.sampler import load_inference_model
    from .VarAutoEncoder.utils import gpu
    try:
        model = load_inference_model(args.model_output, gpu(args.device), args.checkpoint, ema=args.ema)
    except ValueError as e:
        if not args.ema:
            raise
        raise SystemExit("--ema: {}".format(e))
    cfg = model.engine_config
    gen = LatentGenerator(model, seed=args.seed, temperature=args.temperature, decoder=args.decoder, beam_size=args.beam_size,
                          max_rows=args.max_rows, sample_temperature=args.sample_temperature, top_k=args.top_k, top_p=args.top_p)
    if args.mode == "prior":
        classes = args.classes if args.classes else np.arange(args.n) % cfg.num_classes
        out = gen.prior(args.n, classes, args.length or 2 * args.max_seq_len)
    else:
        batch = _first_batch(args, cfg.kind)
        if args.mode == "posterior":
            out = gen.posterior(batch, args.n, length=args.length)
        elif args.mode == "interpolate":
            out = gen.interpolate(batch, args.pair[0], args.pair[1], args.steps, mode=args.interpolation, length=args.length)
        elif args.mode == "transfer":
            out = gen.transfer(batch, args.classes or None, length=args.length)
        elif args.mode == "continue":
            out = gen.continue_(batch, args.prime, args.n, args.classes or None, length=args.length)
        elif args.mode == "repaint":
            piece, lens, token = gen._piece(batch)
            if token and args.keep_pitch is not None:
                raise SystemExit("--keep-pitch names piano-roll pitches; a token model keeps --keep-time A B")
            keep = hold_mask(lens, piece.shape[1], None if token else piece.shape[2], time=args.keep_time, pitch=args.keep_pitch)
            out = gen.repaint(batch, keep, args.classes or None, length=args.length)
        elif args.mode == "likelihood":
            lines = likelihood_lines(model, batch, args.iw_samples)
            print("\n".join(lines))
            return lines
        elif args.mode == "score":
            out = gen.score(batch, args.classes or None)
            lines = ["melody {} class {} nll {:.6f}".format(r["melody"], r["cls"], float(s)) for r, s in zip(out.rows, out.held_scores)]
            print("\n".join(lines))
            return lines
        else:
            ca, cb = (args.classes if args.classes and len(args.classes) == 2 else (0, cfg.num_classes - 1))
            out = gen.class_blend(batch, ca, cb, np.linspace(0.0, 1.0, args.steps), length=args.length)
    files = out.write(args.out)
    print("wrote {} files to {}".format(len(files), args.out))
    return files


if __name__ == "__main__":
    main()
