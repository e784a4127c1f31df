"""learn_priors_and_spectra on the fixture's 2 597 rows, batch 64 (41 steps per epoch, one partial row) and batch 448 (6 steps per epoch,
7 partial rows): the call to its return (it reads the losses back), after a warm-up call; microseconds per step (step + update launch)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from tests.posterior_cases import golden, model_for, rows
dev = torch.device("cuda")
data, ratio = rows(dev), float(golden()["epochs3_ratio"])
for batch, epochs in ((64, 50), (448, 300)):
    model_for(torch.float32, device=dev, perturbed=True).learn_priors_and_spectra(data, 2, ratio, batch_size=batch)
    torch.cuda.synchronize()
    out = []
    for _ in range(3):
        m = model_for(torch.float32, device=dev, perturbed=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.learn_priors_and_spectra(data, epochs, ratio, batch_size=batch)
        torch.cuda.synchronize()
        steps = epochs * -(-2597 // batch)
        out.append(1e6 * (time.perf_counter() - t0) / steps)
    print(f"posterior batch {batch}: {steps} steps, us per step " + " ".join(f"{x:.2f}" for x in out), flush=True)
