#!/usr/bin/env python3
"""Generate the ragged-batch fixtures of the original SuDoRM-RF from the REAL reference (build host only).

For every case of tests/original_ragged_fixtures.py: loads the unmodified reference module by file path, puts the case's weights
into it and runs it on EACH ROW ALONE, at the row's own length, batch 1, on CPU in fp32.  Stores wav, lengths and the per-row
outputs (out0 .. out5, each [S, length]) in tests/golden/orig_ragged_<case>.npz.  Asserted here: tests/original_ref.py in fp64
agrees with the reference within 1e-5 on every row, and every row's max |out| lies in [0.1, 10] (so that an absolute bar of 1e-4
means something; a seed that does not give that is replaced, the window is not widened).

    SRF_REFERENCE=<reference checkout> python tools/make_golden_original_ragged.py
Regenerating is bit-identical."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_original import REF, load_ref  # noqa: E402
from tests import original_fixtures as of  # noqa: E402
from tests import original_ragged_fixtures as rf  # noqa: E402
from tests import original_ref as orf  # noqa: E402


def main():
    if not REF or not os.path.isdir(REF):
        raise SystemExit("set SRF_REFERENCE to a checkout of the reference implementation")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    ref = load_ref()
    for name, (cfg, T, lengths, wseed, _) in rf.CASES.items():
        torch.manual_seed(0)
        m = ref.SuDORMRF(**cfg).eval()
        sd = of.make_state_dict(cfg, wseed)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == of.schema(cfg), name
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        wav = rf.make_wav(name)
        arrays = {"wav": wav, "lengths": np.asarray(lengths, dtype=np.int32)}
        for b, n in enumerate(lengths):
            row = wav[b:b + 1, :, :n]
            with torch.no_grad():
                out = m(torch.from_numpy(row)).numpy()
            assert out.shape == (1, cfg["num_sources"], n), (name, b, out.shape)
            amax = float(np.abs(out).max())
            assert 0.1 <= amax <= 10.0, (name, b, amax)
            err = float(np.abs(orf.forward(cfg, sd, row, torch.float64).numpy() - out).max())
            assert err <= 1e-5, (name, b, err)
            arrays["out%d" % b] = out[0]
            print("%s row %d: %5d samples, %3d frames, max|out| %.3f, fp64 restatement %.2e" % (name, b, n, of.frames(cfg, n), amax, err),
                  flush=True)
        of.save_npz(rf.path(name), arrays)
        size = os.path.getsize(rf.path(name))
        assert size <= (1 << 20), (name, size)
        print("wrote %s (%d bytes)" % (rf.path(name), size))


if __name__ == "__main__":
    main()
