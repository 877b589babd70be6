"""python -m clm_gs_amd.eval_mesh -i <mesh.ply> -r <reference.ply> --tau T [T ...] [--spacing S] [--max_distance D]
[--bounds ...] [--ref_every K] [--cell H] [--grid_gb G] [--max_samples N] [-o eval.json] [--error_mesh err.ply]: the command
line of mesh_eval.py ("Mesh evaluation")."""
import sys

from .mesh_eval import main

if __name__ == "__main__":
    sys.exit(main())
