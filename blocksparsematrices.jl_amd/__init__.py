"""MI355X-native block-sparse mat-vec engine: drop-in for the mul! hot path of
djukic14/BlockSparseMatrices.jl (BlockSparseMatrix / SymmetricBlockMatrix / VBCRS x vector).

The directory name contains a dot, so import it through the root-level shim:  `import bsm_amd`.

matrices.py: the operator types and products; entries.py: A[I, J], diag and the COO / CSR export; solvers.py: the
block-Jacobi preconditioner and the Krylov solvers; _marshal.py: the argument marshalling they share; _lib.py: the C ABI.
"""
from . import _lib  # noqa: F401
from . import entries, matrices, solvers, synthetic  # noqa: F401
from .entries import *  # noqa: F401,F403
from .matrices import *  # noqa: F401,F403
from .solvers import *  # noqa: F401,F403
from .solvers import Lsqr, LsqrInfo, Minres, lsqr, minres  # noqa: F401
from .solvers import eigh_blocks, spectral_blocks  # noqa: F401
from .solvers import (PolynomialPreconditioner, chebyshev, chebyshev_coefficients, lanczos_bounds, neumann,  # noqa: F401
                      polynomial)
from .solvers import Eigsh, EigshInfo, eigsh, krylov_combine, krylov_combine_tile  # noqa: F401
from .solvers import (Lobpcg, LobpcgInfo, lobpcg, block_gram, block_gram_grid, block_gram_work, block_combine,  # noqa: F401
                      block_combine_tile)
from .solvers import Svds, SvdsInfo, svds  # noqa: F401

__all__ = matrices.__all__ + entries.__all__ + solvers.__all__ + ["synthetic"]
