"""python -m clm_gs_amd.clean_mesh -i <mesh.ply> -o <out.ply> [--min_faces N] [--keep_largest K] [--decimate_cell C]
[--smooth_iterations N --smooth_lambda L --smooth_mu M] [--normals]: the command line of mesh_clean.py, mesh_smooth.py and
mesh_decimate.py ("Mesh cleanup", "Mesh smoothing and normals" and "Mesh decimation")."""
import sys

from .mesh_clean import main

if __name__ == "__main__":
    sys.exit(main())
