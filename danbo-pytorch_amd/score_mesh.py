"""Score meshes that are already on disk: every .ply of --pred against the file of the same name in --gt, on the GPU
(core/mesh_score.py: Chamfer distance, F-score, normal consistency from area-weighted surface samples and an exact nearest-neighbour
sweep).  Writes mesh_scores.npy ([N, 4 + 3 T]: chamfer_l1, chamfer_l2, normal_consistency, n_points, then precision, recall, fscore
of every threshold in the order given; rows in the sorted order of the file names, listed in mesh_score_names.txt) and
mesh_score_final.txt (the column means) into --out (default: --pred), and prints one line per mesh."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from core import mesh_score  # noqa: E402


def config_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument('--pred', type=str, required=True, help='directory of the predicted meshes (*.ply)')
    p.add_argument('--gt', type=str, required=True, help='directory of the meshes they are scored against, paired by file name')
    p.add_argument('--out', type=str, default=None, help='where the tables go (default: --pred)')
    p.add_argument('--points', type=int, default=100_000, help='surface samples per mesh')
    p.add_argument('--tau', nargs='+', type=float, default=[0.01, 0.02], help='distance thresholds of precision / recall / F-score')
    p.add_argument('--seed', nargs=2, type=int, default=[0, 1], help='seeds of the samples of the prediction and of the ground truth')
    return p


def score_dirs(pred, gt, out=None, points=100_000, tau=(0.01, 0.02), seed=(0, 1)):
    """-> (names, table [N, 4 + 3 T]); a prediction without its file in `gt` is an error that names the file"""
    if not torch.cuda.is_available():
        raise RuntimeError("score_mesh.py drives the HIP kernels: no GPU visible")
    names = sorted(n for n in os.listdir(pred) if n.endswith('.ply'))
    if not names:
        raise FileNotFoundError(f"--pred: no .ply file in {pred}")
    for n in names:
        if not os.path.isfile(os.path.join(gt, n)):
            raise FileNotFoundError(f"--gt: {os.path.join(gt, n)} not found")
    tau, rows = tuple(float(t) for t in tau), []
    for n in names:
        s = mesh_score.score_meshes(os.path.join(pred, n), os.path.join(gt, n), n_points=points, thresholds=tau, seed=tuple(seed))
        rows.append(mesh_score.score_row(s, points, tau))
        print(mesh_score.score_line(n[:-4], s, tau))
    out = pred if out is None else out
    os.makedirs(out, exist_ok=True)
    table = mesh_score.save_scores(out, rows, tau)
    with open(os.path.join(out, 'mesh_score_names.txt'), 'w') as f:
        f.write("".join(n + "\n" for n in names))
    return names, table


def main(argv=None):
    a = config_parser().parse_args(argv)
    return score_dirs(a.pred, a.gt, a.out, a.points, a.tau, a.seed)


if __name__ == '__main__':
    main()
