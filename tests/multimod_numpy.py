"""numpy restatement of nnetRNNMultimod as speech_recognition_tools_amd/multimod.py runs it (tests/test_multimod.py),
in float64 or float32, on tests/gru_numpy.py: stream s's rows through sub-network s (GRU layers), the outputs side by
side through the trunk GRUs, then the regression.  Layers are (w_ih, w_hh, b_ih, b_hh) as MultimodPlan takes them.
"""
import numpy as np

import gru_numpy as GN


def forward(rows, subnets, trunk, regression, dtype=np.float64):
    """rows[s]: stream s's [T, K] rows of one utterance.  Returns (sub [M][T, Hs], the last layer of every
    sub-network; trunk [Lt][T, M Hs]; logits [T, C])."""
    sub = []
    for x, sn in zip(rows, subnets):
        h = np.asarray(x).astype(dtype)
        for layer in sn:
            h = GN.gru_layer(h, *layer, dtype=dtype)
        sub.append(h)
    h, outs = np.concatenate(sub, axis=1), []
    for layer in trunk:
        h = GN.gru_layer(h, *layer, dtype=dtype)
        outs.append(h)
    w, b = regression
    return sub, outs, h @ np.asarray(w).astype(dtype).T + np.asarray(b).astype(dtype)
