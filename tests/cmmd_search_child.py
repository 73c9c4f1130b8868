"""Child process of tests/test_hip_cmmd.py: scripts/sd_search_ea.py's main() under a process group of this one rank, with two
observers -- every candidate's fitness with the embedding rows it was computed from, and every pooled_rows call with what went in,
what came out and over which backend -- written to an .npz.

    python tests/cmmd_search_child.py OUT.npz <flags of scripts/sd_search_ea.py>

A process of its own because it initialises a process group (one per process)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    out, argv = sys.argv[1], sys.argv[2:]
    import torch.distributed as dist
    from autodiffusion_amd import cmmd, dist_util, sd_evaluate
    dist_util.setup_dist()          # RANK 0 of WORLD_SIZE 1; ADM_FORCE_COLLECTIVES=1 sends the pooling through the backend all the same
    fits, pools = [], []
    fit0, pool0 = sd_evaluate.SDCandidateEvaluator.get_cand_fid, cmmd.pooled_rows

    def fit(self, cand=None, opt=None, device=None):
        v = fit0(self, cand, opt, device)
        rows = self.last_rows
        fits.append((np.zeros((0, 0), np.float32) if rows is None else rows.detach().cpu().numpy().copy(), float(v),
                     self.features is None))
        return v

    def pool(rows, group=None, local=False):
        res = pool0(rows, group, local)
        through = bool(dist_util.collectives_on(group)) and not local
        pools.append((rows.detach().cpu().numpy().copy(), res.detach().cpu().numpy().copy(), through,
                      dist.get_backend() if dist.is_initialized() else "", str(res.device)))
        return res

    sd_evaluate.SDCandidateEvaluator.get_cand_fid = fit
    cmmd.pooled_rows = pool          # the evaluator looks the name up at call time
    spec = importlib.util.spec_from_file_location("sd_search_ea_cli", os.path.join(ROOT, "scripts", "sd_search_ea.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    searcher = cli.main(argv)
    data = {"count": np.array(len(fits)), "no_extractor": np.array(all(f[2] for f in fits) and searcher.evaluator.features is None)}
    for i, (rows, v, _) in enumerate(fits):
        data[f"rows{i}"], data[f"value{i}"] = rows, np.array(v)
    for i, (a, b, through, backend, device) in enumerate(pools):
        data[f"pool_in{i}"], data[f"pool_out{i}"] = a, b
        data[f"pool_how{i}"] = np.array([str(through), backend, device])
    np.savez(out, **data)
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
