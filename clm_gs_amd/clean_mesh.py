"""python -m clm_gs_amd.clean_mesh -i <mesh.ply> -o <out.ply> [--min_faces N] [--keep_largest K]: the command line of
mesh_clean.py ("Mesh cleanup")."""
import sys

from .mesh_clean import main

if __name__ == "__main__":
    sys.exit(main())
