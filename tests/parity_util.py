"""Helpers shared by the parity tests: run the same synthetic streams through
the CPU oracle (checker) and through the HIP engine (product)."""
import functools

import numpy as np

FRAME = 480

# ---------------- test models (rnnoise text format) ----------------

# text-file layer order: (nb_inputs, nb_neurons, activation text code, gru);
# the codes are the upstream model's and fvad_model_synthetic's
LAYERS = [(42, 24, 0, False), (24, 24, 2, True), (90, 48, 2, True), (114, 96, 2, True), (96, 22, 1, False),
          (24, 1, 1, False)]
N_WEIGHTS = 87503

# one permutation of the activation text codes (0 tanh, 1 sigmoid, 2 relu) in
# LAYERS order: no layer keeps the code it has in LAYERS
PERMUTED_ACTS = (1, 0, 1, 0, 0, 2)
# ... and the third code of every layer.  With PERMUTED_ACTS the relu vad_output
# is 0 on every frame of every synthetic stream (its sum never turns
# positive), so that assignment checks the vad branch's codes through the
# denoised output only; with this one vad moves on every frame.
PERMUTED_ACTS_B = (2, 1, 0, 1, 2, 0)


def write_text_model(blob, path, acts=None):
    """Write a blob (fvad_model_blob order) as an rnnoise text model; acts
    replaces the six layers' activation codes."""
    lines = ["rnnoise-nu model file version 1"]
    o = 0
    for k, (nin, nout, act, gru) in enumerate(LAYERS):
        g = 3 if gru else 1
        sizes = [nin * nout * g] + ([nout * nout * 3] if gru else []) + [nout * g]
        lines.append("%d %d %d" % (nin, nout, act if acts is None else acts[k]))
        for n in sizes:
            lines.append(" ".join(str(int(v)) for v in blob[o:o + n]))
            o += n
    path.write_text("\n".join(lines) + "\n")


_M64 = (1 << 64) - 1


def _splitmix64(seed, n):
    """n outputs of fvad_model.cpp's mix(), the state starting at seed (Python integers only)."""
    s = seed & _M64
    for _ in range(n):
        s = (s + 0x9E3779B97F4A7C15) & _M64
        z = s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        yield z ^ (z >> 31)


def _w_trained_like(z):
    # magnitudes 16 * geometric + uniform(16): most weights small, a tail
    # clipped at both ends of int8, as a trained rnnoise model's are
    lo = z & 0xFFFFFFFF
    m = 16 * (32 - lo.bit_length()) + ((z >> 32) % 16)
    if z >> 63:
        m = -m
    return max(-128, min(127, m))


# name -> (splitmix64 seed, weight from one draw z)
TEST_MODELS = {
    "trained_like": (2, _w_trained_like),
    "uniform_full": (3, lambda z: (z % 256) - 128),
    "extremes": (4, lambda z: 127 if z & 1 else -128),
}


@functools.lru_cache(maxsize=None)
def _model_blob(name):
    seed, weight = TEST_MODELS[name]
    b = np.array([weight(z) for z in _splitmix64(seed, N_WEIGHTS)], np.int8)
    b.setflags(write=False)
    return b


def model_blob(name):
    """The int8 weights of a test model, in fvad_model_blob order (read-only, cached)."""
    return _model_blob(name)


# the model-domain tests' cases: id -> (weights, activation codes); weights
# "seed1" are fvad_model_synthetic(1)'s, acts None the codes of LAYERS
DOMAIN_MODELS = {
    "trained_like": ("trained_like", None),
    "uniform_full": ("uniform_full", None),
    "extremes": ("extremes", None),
    "trained_like-acts": ("trained_like", PERMUTED_ACTS),
    "seed1-acts": ("seed1", PERMUTED_ACTS),
    "trained_like-actsB": ("trained_like", PERMUTED_ACTS_B),
    "seed1-actsB": ("seed1", PERMUTED_ACTS_B),
}


def write_domain_model(fvad, case, tmp_path):
    """Write one of DOMAIN_MODELS as a text file under tmp_path: (path, blob)."""
    weights, acts = DOMAIN_MODELS[case]
    blob = fvad.Model(seed=1).blob() if weights == "seed1" else model_blob(weights)
    path = tmp_path / (case + ".txt")
    write_text_model(blob, path, acts)
    return str(path), blob


# the model-domain tests' streams (synth_stream id, seconds), stereo: ragged
# lengths that are no multiple of 480 samples, stream 19 with its digital
# silence at 5 s, and three streams so every GRU kernel has a partial workgroup
DOMAIN_STREAMS = ((0, 2.5), (19, 6.5), (42, 3.3))


def domain_streams(fvad):
    return [fvad.synth_stream(i, int(48000 * s), 2)[0] for i, s in DOMAIN_STREAMS]


def sensitivity_probe(oracle, om, x, frame=10, delta=0.01):
    """Run the oracle Denoiser twice over x (mono, s16 units), the second time
    with delta added to one sample of the given frame: (max |dvad|, denoised
    rel-RMS) between the two runs.  How far one rounding error in the input
    moves the outputs -- whether a model is tame enough for a tolerance test."""
    runs = []
    for d in (0.0, delta):
        y = np.array(x, np.float32)
        y[frame * FRAME + FRAME // 2] += np.float32(d)
        den = oracle.Denoiser(om)
        res = [den.process(y[i * FRAME:(i + 1) * FRAME]) for i in range(len(y) // FRAME)]
        runs.append((np.concatenate([r[0] for r in res]).astype(np.float64), np.array([r[1] for r in res])))
    (a, va), (b, vb) = runs
    rel = float(np.sqrt(np.mean((a - b) ** 2)) / max(1e-12, np.sqrt(np.mean(a ** 2))))
    return float(np.abs(va - vb).max()), rel



def make_streams(fvad, ids, seconds, n_channels=2):
    out, labels = [], []
    for sid in ids:
        x, lab = fvad.synth_stream(sid, int(48000 * seconds), n_channels)
        out.append(x)
        labels.append(lab)
    return out, labels


def oracle_run(oracle, om, streams, denoised=True):
    res = []
    for x in streams:
        Ch, n = x.shape
        frames = n // FRAME
        p = oracle.Pipeline(Ch, om, trace_frames=frames + 1, trace_windows=frames // 4 + 2,
                            trace_denoised=(frames * FRAME if denoised else 0))
        for k in range(0, n, 48000):
            p.push([x[c, k:k + 48000] for c in range(Ch)])
        fr, wi = p.trace()
        res.append({"frames": fr, "windows": wi, "segments": p.segments(),
                    "denoised": p.tden[:, : frames * FRAME].copy() if denoised else None})
    return res


def engine_run(fvad, engine, streams, chunk_ticks, denoised=True):
    B = len(streams)
    Ch = streams[0].shape[0]
    lens = [x.shape[1] // FRAME for x in streams]
    T = max(lens)
    outs = []
    for t0 in range(0, T, chunk_ticks):
        nt = min(chunk_ticks, T - t0)
        pcm = np.zeros((nt, B, Ch, FRAME), np.float32)
        valid = np.zeros(B, np.int32)
        for s, x in enumerate(streams):
            v = max(0, min(nt, lens[s] - t0))
            valid[s] = v
            if v:
                seg = x[:, t0 * FRAME:(t0 + v) * FRAME].reshape(Ch, v, FRAME)
                pcm[:v, s] = seg.transpose(1, 0, 2)
        outs.append((engine.push(pcm, ticks_valid=valid, denoised=denoised), valid))
    W = getattr(engine, "wpt", 1)
    per = []
    for s in range(B):
        vad, ratio, wf, wr, wv, band, den = [], [], [], [], [], [], []
        for o, valid in outs:
            v = valid[s]
            cnt = o["win_flag"][:v, s]
            vad.append(o["vad"][:v, s])
            ratio.append(o["ratio"][:v, s])
            wf.append(cnt)
            wr.append(tick_windows(o["win_ratio"][:v, s], cnt, W))
            wv.append(tick_windows(o["win_vad"][:v, s], cnt, W))
            band.append(tick_windows(o["band"][:v, s], cnt, W))
            if denoised:
                den.append(o["denoised"][:v, s])
        r = {"vad": np.concatenate(vad), "ratio": np.concatenate(ratio), "win_flag": np.concatenate(wf),
             "win_ratio": np.concatenate(wr), "win_vad": np.concatenate(wv), "band": np.concatenate(band)}
        if denoised:
            d = np.concatenate(den)  # [T][Ch][480]
            r["denoised"] = d.transpose(1, 0, 2).reshape(Ch, -1)
        per.append(r)
    return per


def tick_windows(x, counts, W):
    """The completed windows of one stream's ticks, in sample order: x is
    [ticks]... (W == 1) or [ticks][W]... (window slots), counts the ticks'
    win_flag (windows completed per tick)."""
    counts = np.asarray(counts)
    if W == 1:
        return x[counts.astype(bool)]
    return x[np.arange(W)[None, :] < counts[:, None]]


def first_mismatch(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    ne = np.nonzero(a.reshape(-1) != b.reshape(-1))[0]
    return int(ne[0]) if len(ne) else -1
