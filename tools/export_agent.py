"""Export a trained reference agent -> tests/golden/<model>_bdq_final.npz (fp32 tensors).

    python tools/export_agent.py pbn7 bb33 pbn10     (build container only: reads /root/reference)

models/<model>/bdq_final.pt is the BranchingDQN state dict the reference saves at the end of
training (bdq_model/__init__.py:237,240-244) and model_tester.py:548-549 evaluates.  It is
loaded with torch.load(weights_only=True) (tensors only, nothing executed) and the ``q.``
network's tensors are written under their BranchingQNetwork names, so that the GPU box (which
has no /root/reference) can rebuild the agent.  The law pins replay model_tester.py:587-658
with them (tests/test_law_pin.py, tests/test_bn_pin.py, tests/test_gpu_law_pin.py).
"""
import os
import sys

import torch

REF = "/root/reference"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tests.golden_parts import save_parts  # noqa: E402


def export(model: str) -> str:
    sd = torch.load(os.path.join(REF, "models", model, "bdq_final.pt"), map_location="cpu", weights_only=True)
    q = {k[2:]: v.detach().to(torch.float32).numpy() for k, v in sd.items() if k.startswith("q.")}
    out = os.path.join(GOLD, f"{model}_bdq_final.npz")
    print("wrote", save_parts(out, q), sum(v.size for v in q.values()), "floats")   # parts below 1 MiB
    return out


def export_ddqn(pt_path: str, out: str) -> str:
    """python tools/export_agent.py --ddqn ddqn_25000.pt ddqn_25000.npz: a reference DDQN / DDQNPER
    save dict (ddqn_per/__init__.py:130-153; a pickled dict, so load only your own files) as the arrays
    pbn_rl_amd.ddqn.load_ddqn_checkpoint reads: params.<name>, net_arch, input_size, output_size."""
    import numpy as np
    sd = torch.load(pt_path, map_location="cpu", weights_only=False)
    arrays = {"params." + k: v.detach().to(torch.float32).numpy() for k, v in sd["params"].items()}
    arrays["net_arch"] = np.array(sd["policy_kwargs"]["net_arch"], dtype=np.int64).reshape(-1, 2)
    arrays["input_size"] = np.int64(sd["input_size"])
    arrays["output_size"] = np.int64(sd["output_size"])
    np.savez(out, **arrays)
    print("wrote", out, sum(v.size for v in arrays.values()), "values")
    return out


if __name__ == "__main__":
    if sys.argv[1:2] == ["--ddqn"]:
        export_ddqn(sys.argv[2], sys.argv[3])
    else:
        for m in sys.argv[1:] or ["pbn7"]:
            export(m)
