from .trajectories import get_optical_flow_tile_mask, coeffs_grid_to_list  # noqa: F401
from .basis import compute_basis, basis_values, basis_table, table_basis_values, bernstein_basis, trajectories_from_bezier, bspline_basis, trajectories_from_bspline, flows_from_bezier, curve_basis, trajectories_from_curves, flows_from_curves, curve_event_basis, curve_head_rows  # noqa: F401
from .event_image_converter import EventImageConverter  # noqa: F401
from .voxel_grid import VoxelGrid, voxel_grids  # noqa: F401
from .ingest import ingest_events, ingest_raw_events  # noqa: F401
from .flow import dense_flow_from_traj, calculate_flow_error, ErrorCalculatorFactory, OpticalFlowError  # noqa: F401
from .grid_traj import trajectories_from_grid, flow_from_grid  # noqa: F401
from . import representation  # noqa: F401  (representation.VoxelGrid is the EVIMO2 / MultiFlow class; VoxelGrid above is the DSEC one)
from .representation import representation_grids  # noqa: F401
from .val_metrics import trajectory_val_metrics, TrajectoryValMetrics, val_metric_keys  # noqa: F401
from .flow_targets import flow_targets  # noqa: F401
from .dsec_io import dsec_flow_targets, dsec_flow_error, dsec_flow_png16  # noqa: F401
from .corr import corr_pyramid, corr_pyramid_fused, CorrLookup, coords_grid, level_target_indices  # noqa: F401
