"""The network's coefficient grid -> `trajectories` for FocusLoss.calc, as the reference's training step builds them (row A3 of
SURVEY.md 8(a)): TrajectoryNet.calculate_trajectories_at_t and calculate_flow (reference src/modules/trajectory_net.py:57-140) with
the standard tile mask.  On the GPU one autograd node (ops.GridTrajFn, csrc/grid_traj.hip); elsewhere the plain-torch mirror
(coeffs_grid_to_list + compute_basis), as `_curve_trajectories` does for the curve adapters."""
import torch

from .basis import compute_basis
from .trajectories import get_optical_flow_tile_mask, coeffs_grid_to_list
from . import flow as _flow

_BASIS_CODE = {'polynomial': 0, 'dct': 1, 'learned': 2}          # include/mpcmax.h: MPC_BASIS_POLY / _DCT / _MATRIX
_GRID_POS_CACHE = {}
GRID_KMAX = 16
GRID_DTYPES = (torch.float32, torch.float16, torch.bfloat16)          # what the kernels read in place (include/mpcmax.h: MPC_DT_*)
GRID_PHI_FLOATS = 4096          # n_t * k limit of the kernels (csrc/grid_traj.hip: GT_PHI_BYTES, the LDS slice of the basis)


def grid_tile_counts(H, W, tile_size):
    """(hq, wq): the tile rows and columns of get_optical_flow_tile_mask((H, W), tile_size) -- the count of mask[s::tile, s::tile],
    ceil((H - tile // 2) / tile), which differs from ceil(H / tile) where H is not a multiple of the tile size."""
    s = tile_size // 2
    return (max(0, -(-(H - s) // tile_size)), max(0, -(-(W - s) // tile_size)))


def _grid_positions(H, W, tile_size, device):
    """The tile centres [n, 2] (y, x) int64 on `device`, row-major (= torch.nonzero of the tile mask), built once per
    (H, W, tile, device) on the device itself (no upload: no host synchronisation inside a step)."""
    key = (int(H), int(W), int(tile_size), str(device))
    pos = _GRID_POS_CACHE.get(key)
    if pos is None:
        if len(_GRID_POS_CACHE) > 16:
            _GRID_POS_CACHE.clear()
        hq, wq = grid_tile_counts(H, W, tile_size)
        s = tile_size // 2
        ys = torch.arange(hq, dtype=torch.int64, device=device) * tile_size + s
        xs = torch.arange(wq, dtype=torch.int64, device=device) * tile_size + s
        pos = _GRID_POS_CACHE[key] = torch.stack((ys[:, None].expand(hq, wq), xs[None, :].expand(hq, wq)), -1).reshape(hq * wq, 2)
    return pos


def trajectories_from_grid(coeff_grid, times, num_basis, basis_type, tile_size, add_offsets=True, basis_network=None, anchor_time=0.0):
    """TrajectoryNet.calculate_trajectories_at_t(coeff_grid, times, object_mask, add_offsets) of the reference (trajectory_net.py:
    101-119) with the standard tile mask of patch_size = tile_size, for the training loop to call in its place.

    coeff_grid [B, S, 2k, H, W] (or [B, 2k, H, W] as S = 1; channels 0..k-1: y, k..2k-1: x; the scales are summed), times [n_t] (on
    the grid's device: FocusLoss.get_reconstruction_times draws t_ref there every step), basis_type 'polynomial' (t^j), 'dct'
    (sqrt(2) cos(pi/2 (2t + 1) j)) or 'learned' (basis_network(times[..., None]) -> [n_t, k]), j = 1..k; the basis at anchor_time is
    subtracted (the reference's anchor is 0).  Returns (trajectories [B, n_t, n, 2] (y, x), pixel_positions [n, 2] int64 (y, x) on the
    grid's device) -- tile centres (tile // 2 + iy * tile, tile // 2 + ix * tile), row-major.  `pixel_positions` is a cached tensor
    shared by all calls of the same (H, W, tile, device): do not modify it in place.

    A CUDA grid in fp32, fp16 or bf16 with 1 <= k <= 16 and n_t * k <= 4096 runs one kernel forward and one backward (two for
    'learned', whose [n_t, k] basis difference keeps its gradient, so the MLP trains), on torch's current stream, without a host
    synchronisation, fp32 contiguous trajectories.  A 16-bit grid (a network under autocast, a .half() / .bfloat16() model) is read
    as it is -- no .float() copy; the conversion at the load is exact, so the trajectories are, bit for bit, those of grid.float()
    -- and its gradient comes back in the grid's dtype, computed in fp32 and rounded once.  The trajectories of a CUDA 16-bit grid
    are therefore fp32, NOT the grid's dtype as they were when such a grid took the mirror: displacement + pixel position in bf16
    (8 significant bits) puts positions between 256 and 640 px on a 2-4 px lattice, which is useless to the loss.  Anything else
    -- CPU tensors, other dtypes, k > 16, more than 4096 basis values n_t * k -- takes the plain-torch mirror (coeffs_grid_to_list +
    compute_basis), which returns the dtype of the grid.  Object masks other than the tile mask are not served here: use
    coeffs_grid_to_list and compute_basis with the mask, as the reference does."""
    if coeff_grid.dim() == 4:
        coeff_grid = coeff_grid[:, None]                        # trajectory_net.py:113-114
    B, S, c2, H, W = coeff_grid.shape
    k, tile = int(num_basis), int(tile_size)
    if basis_type not in _BASIS_CODE:
        raise ValueError(basis_type)
    if c2 != 2 * k:
        raise ValueError(f'coeff_grid has {c2} channels, 2 * num_basis = {2 * k} expected')
    dev = coeff_grid.device
    pos = _grid_positions(H, W, tile, dev)
    if coeff_grid.is_cuda and coeff_grid.dtype in GRID_DTYPES and 1 <= k <= GRID_KMAX and times.numel() * k <= GRID_PHI_FLOATS:
        from .. import ops
        if times.device != dev:
            times = times.to(dev)
        dphi = None
        if basis_type == 'learned':
            anchor = torch.full((1,), float(anchor_time), device=dev, dtype=times.dtype)
            dphi = basis_network(times[..., None]) - basis_network(anchor[..., None])       # [n_t, k]
        return ops.GridTrajFn.apply(coeff_grid, times, dphi, _BASIS_CODE[basis_type], float(anchor_time), bool(add_offsets), tile), pos
    # the mirror: calculate_coords (trajectory_net.py:101-111) on coeffs_grid_to_list's gather
    mask = get_optical_flow_tile_mask((H, W), tile).to(dev)
    coeffs, positions, _ = coeffs_grid_to_list(coeff_grid, mask, k)
    anchor = torch.full((1,), float(anchor_time), device=dev, dtype=coeffs.dtype)
    traj = compute_basis(coeffs, times, k, basis_type, basis_network) - compute_basis(coeffs, anchor, k, basis_type, basis_network)
    if add_offsets:
        traj = traj + positions[None, :, None, :]
    return traj.permute(0, 2, 1, 3).contiguous(), pos


def flow_from_grid(coeff_grid, num_basis, basis_type, tile_size, image_shape, t_end=1.0, basis_network=None):
    """TrajectoryNet.calculate_flow of the reference (trajectory_net.py:121-140): the displacement of every tile from the anchor 0 to
    t_end (1, or 1 / skip_frames) through trajectories_from_grid (add_offsets=False), spread to a dense flow [B, 2, H, W] (y, x) by
    utils.dense_flow_from_traj (a GPU operator: csrc/flow.hip)."""
    if coeff_grid.dim() == 4:
        coeff_grid = coeff_grid[:, None]
    times = torch.full((1,), float(t_end), device=coeff_grid.device, dtype=torch.float32)
    traj, pos = trajectories_from_grid(coeff_grid, times, num_basis, basis_type, tile_size, add_offsets=False, basis_network=basis_network)
    dense, _ = _flow.dense_flow_from_traj(traj[:, 0], pos, tile_size, image_shape)
    return dense
