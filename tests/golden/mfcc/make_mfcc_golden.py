#!/usr/bin/env python3
"""Generate the MFCC front end's fixture from the REFERENCE's data files.

Run in the build container only (needs /root/reference, read-only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/mfcc/make_mfcc_golden.py

Writes DATA only, next to this script (a subdirectory: tests/conftest.py feeds every top-level tests/golden/*.npz to
the single-layer fixtures):

* reference_clip.npz -- ``pcm``: the 16 000 int16 samples of scratch/down_sample.wav (16 kHz mono, one second, the word
  "down"); ``mean`` / ``std``: model_batchnorm/mean.npy / std.npy squeezed to 64 values each (inferencetry.py:297-300:
  32 MFCC + 32 delta); ``classes``: the 12 class names of the trained keyword spotter's label encoder, in index order
  (class 0 is "down").
"""
import os
import sys

import numpy as np
import torch
from scipy.io import wavfile

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


def main():
    sr, pcm = wavfile.read(os.path.join(REF, "scratch", "down_sample.wav"))
    assert sr == 16000 and pcm.dtype == np.int16 and pcm.shape == (16000,), (sr, pcm.dtype, pcm.shape)
    mean = np.squeeze(np.load(os.path.join(REF, "model_batchnorm", "mean.npy"))).astype(np.float32)
    std = np.squeeze(np.load(os.path.join(REF, "model_batchnorm", "std.npy"))).astype(np.float32)
    assert mean.shape == (64,) and std.shape == (64,)
    ckpt = torch.load(os.path.join(REF, "model_batchnorm", "FastGRNNBatchNorm_KeywordSpotter.pt"), map_location="cpu",
                      weights_only=False)
    classes = [str(c) for c in ckpt["label_encoder"].classes_.tolist()]
    assert len(classes) == 12
    np.savez_compressed(os.path.join(HERE, "reference_clip.npz"), pcm=pcm, mean=mean, std=std,
                        classes=np.array(classes))
    print("reference_clip: peak %d, classes %s" % (int(np.abs(pcm.astype(np.int32)).max()), classes))


if __name__ == "__main__":
    main()
