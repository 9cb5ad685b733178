"""Bitwise A/B of the optimizer entry points between two builds of the library (a tool, not a test): walks the scenarios of
tests/test_gpu_optim_sequence.py — every has-a-gradient state x every update and norm entry, num_tokens 0 and 64 — for three
steps each on a fresh engine, and after every step prints a SHA-256 of params, exp_avg, exp_avg_sq, the norm buffer's four
result floats and, for LAMB, the 4 * PLB_NPARAM result floats of the LAMB buffer. Run it once per library and compare:
   PLBERT_HIP_LIB=/path/to/parent/libplbert_hip.so python tools/optim_entry_ab.py > a.txt
   python tools/optim_entry_ab.py > b.txt && diff a.txt b.txt
(profiles/optim_entry_ab.txt holds one such pair.)"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def main():
    import torch
    from plbert_amd import _lib
    import test_gpu_optim_sequence as T

    if not torch.cuda.is_available():
        raise SystemExit("optim_entry_ab needs the GPU")
    for nt, state in T.STATES:
        for entry in list(T.STEPS) + list(T.NORMS):
            rig = T.Rig(nt)
            eng = rig.eng
            for step in (1, 2, 3):
                rig.backward(state)
                if entry == "norm_partials":
                    eng.grad_accum_add(eng.GRAD_FIRST)
                    rig.backward(state)
                    eng.grad_accum_add(eng.GRAD_LAST, want_partials=True)
                rig.run(entry, step + 1)          # (the rig's warm step was step 1)
                torch.cuda.synchronize()
                sums = [sha(eng.params), sha(eng.exp_avg), sha(eng.exp_avg_sq), sha(eng.norm_buf[:4])]
                if entry.startswith("lamb"):
                    sums.append(sha(eng.lamb_buf[:4 * _lib.PLB_NPARAM]))
                print(f"{nt:2d} {state:8s} {entry:14s} step {step} tok_steps {eng.token_head_steps} " + " ".join(sums), flush=True)


if __name__ == "__main__":
    main()
