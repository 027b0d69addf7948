"""Oracle for the streaming sinc resampler (ctn_stream_resample, include/ctn_hip.h "streaming sinc resampling"): the contract
restated in pure numpy with an explicit history, written from that contract.  No GPU, no import of the package.

    ready(N, up, down, W)               -> E(N): the outputs computable after N input samples
    Stream(up, down, h, W)              one row: .push(samples) -> float32 outputs, .close() -> the flush
    run(x, cuts, up, down, h, W)        -> the concatenation of every push of x cut at `cuts`, and the flush

The row keeps its last 2W - 1 samples and its sample count, nothing else.  The tap sum is resample_oracle's: acc = +0, taps in
ascending order, one float32 rounding per product and per add.
"""
import numpy as np


def ready(N, up, down, W):
    """E(N) = ceil((N - W) * up / down) for N > W, 0 otherwise: output t reads input up to floor(t * down / up) + W."""
    return -((-(int(N) - W) * up) // down) if N > W else 0


class Stream:
    def __init__(self, up, down, h, W):
        assert h.dtype == np.float32 and h.shape == (up, 2 * W)
        self.up, self.down, self.h, self.W = int(up), int(down), h, int(W)
        self.hist = np.zeros(2 * W - 1, dtype=np.float32)      # samples n - (2W - 1) .. n - 1; zeros before sample 0
        self.n = 0                                             # samples received
        self.deepest = 0                                       # how far behind n any tap has reached (a check for the tests)

    def _emit(self, new, t0, t1):
        """Outputs [t0, t1) from the history, the new samples and zeros beyond them."""
        H, W, n_old = 2 * self.W - 1, self.W, self.n
        y = np.zeros(t1 - t0, dtype=np.float32)
        if t1 == t0:
            return y
        t = np.arange(t0, t1, dtype=np.int64)
        pos = t * self.down
        first, phase = pos // self.up - W + 1, pos % self.up    # global index of tap 0
        assert int(first.min()) >= n_old - H, "an output needs a sample older than the history"
        self.deepest = max(self.deepest, n_old - int(first.min()))
        back = max(0, int(first.max()) + 2 * W - (n_old + len(new)))
        line = np.concatenate([self.hist, np.asarray(new, dtype=np.float32), np.zeros(back, dtype=np.float32)])   # line[k] = sample n_old - H + k
        at = first - (n_old - H)
        for j in range(2 * W):
            y = y + self.h[phase, j] * line[at + j]             # one rounding for the product, one for the add
        assert y.dtype == np.float32
        return y

    def push(self, new):
        new = np.asarray(new, dtype=np.float32)
        t0, t1 = ready(self.n, self.up, self.down, self.W), ready(self.n + len(new), self.up, self.down, self.W)
        y = self._emit(new, t0, t1)
        if len(new):
            self.hist = np.concatenate([self.hist, new])[-(2 * self.W - 1):]
            self.n += len(new)
        return y

    def close(self):
        t0, t1 = ready(self.n, self.up, self.down, self.W), -((-self.n * self.up) // self.down)
        return self._emit(np.zeros(0, dtype=np.float32), t0, t1)


def run(x, cuts, up, down, h, W):
    """x cut into consecutive pushes of `cuts` samples (they sum to len(x)) -> (outputs of every push, flush)."""
    assert sum(cuts) == len(x)
    s, at, outs = Stream(up, down, h, W), 0, []
    for k in cuts:
        outs.append(s.push(x[at:at + k]))
        at += k
    return outs, s.close(), s
