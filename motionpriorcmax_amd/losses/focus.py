"""FocusLoss behind the reference's loss plugin API, computed by the HIP kernels of libmpcmax.

Same constructor keys, attributes and `calc` contract as reference src/losses/focus.py:9-113, so
`TrajectoryNet.step` (src/modules/trajectory_net.py:142-161) and the image-logging callback
(src/utils/logging.py:53-120) can use it unchanged."""
import torch

from . import base
from .. import ops
from ..utils.event_image_converter import EventImageConverter


class FocusLoss(base.TrajectoryLossBase):
    """
    Args (reference focus.py:13-27):
        image_shape (tuple): (height, width).
        num_tref (int): number of reference times; 1 = one random reference time.
        num_bins (int): number of time bins of the flow look-up table.
        num_knn (int): nearest trajectories averaged per look-up-table cell.
        smooth_weight (float): weight of the smoothness term.
        lut_superpixel_size (int): pixel size of one look-up-table cell.
        focus_loss_norm (str): 'l1' or 'l2' gradient-magnitude norm.
        dist_norm (str): 'l1' or 'l2' neighbour distance.
        scale_iwe_by_dt, mask_image_border, polarity_aware_batching (bool)
        interpolation_scheme (str): 'mean' or 'iwd'.
        smooth_type (str): 'on_flow_to_tref' or 'on_flow_to_next'.
        loss_type (str, build-side extension): 'gradient_magnitude' (what the reference hard-codes,
            focus.py:90-91) or 'variance' (reference src/utils/loss.py:14-16).
        pyramid_levels (int, UNPINNED extension, default 1 = the reference): IWE pyramid of that many levels, 2 .. 6 -- level l + 1 is
            the 2x2 average of the raw level l, every level goes through the reference's blur and gradient-magnitude objective on its
            own elements, and the focus term is the sum of the levels' 1 / val; `iwes` stay the blurred level-0 images, the smoothness
            term is untouched.  BASELINE.json names one, the reference has none.  Served on EVERY loss route -- `calc` (eager, with
            `event_offsets`, static_shapes and the automatic capture), `calc_per_event_basis`, `calc_per_event_curves` and their
            unfused cross-checks -- by one fused pass behind the route's forward (`ops.iwe_pyramid_pass`: three launches, two without
            a gradient; the backward of the route is unchanged).  Refused with a ValueError: num_tref > 1, loss_type='variance', an
            image not divisible by 2^(levels - 1) or with a coarsest level below 3x3, more than 65535 trajectories per sample.
        pyramid_fused (bool, default True): False sends `calc` through the stage calls of `ops.PyramidFocusFn` instead (one pooling,
            contrast and finalize launch per level, no captured form, `event_offsets` unused): the cross-check of the fused pass.
        trefs_as_samples (bool, build-side switch, default True): with num_tref > 1 the T reference times of a sample run as T samples
            of the num_tref == 1 kernels (`_calc_trefs_as_samples`); False: the general kernels (every stage in one launch for all T).
        static_shapes (bool, build-side extension, default False): capture `calc` + backward once per input shape into HIP
            graphs and replay them (ops.StaticFocusPlan): for small batches, whose eager step is bound by the host.
            `misc_metadata['iwes']` is then only valid until the next `calc`.
    """

    def __init__(self, image_shape, num_tref, num_bins, num_knn, smooth_weight,
                 lut_superpixel_size, focus_loss_norm, dist_norm,
                 scale_iwe_by_dt, mask_image_border, polarity_aware_batching,
                 interpolation_scheme, smooth_type, loss_type='gradient_magnitude', profiler=None,
                 static_shapes=False, pyramid_levels=1, auto_static_shapes=True, trefs_as_samples=True, pyramid_fused=True, **kwargs):
        super().__init__()
        self.image_shape = image_shape
        self.num_tref = num_tref
        self.num_bins = num_bins
        self.num_knn = num_knn
        self.smooth_weight = smooth_weight
        self.lut_superpixel_size = lut_superpixel_size
        self.focus_loss_norm = focus_loss_norm
        self.dist_norm = dist_norm
        self.scale_iwe_by_dt = scale_iwe_by_dt
        self.mask_image_border = mask_image_border
        self.polarity_aware_batching = polarity_aware_batching
        self.interpolation_scheme = interpolation_scheme
        self.smooth_type = smooth_type
        self.loss_type = loss_type
        self.profiler = profiler
        self.static_shapes = bool(static_shapes)
        self.pyramid_levels = int(pyramid_levels)      # UNPINNED extension (ops.iwe_pyramid_pass); 1 = the reference's single scale
        self.pyramid_fused = bool(pyramid_fused)       # False: `calc` on the stage calls of ops.PyramidFocusFn (cross-check)
        if self.pyramid_levels < 1 or (self.pyramid_levels > 1 and (num_tref != 1 or loss_type != 'gradient_magnitude')):
            raise ValueError(f"pyramid_levels > 1 needs num_tref == 1 and the gradient-magnitude objective (got num_tref={num_tref}, "
                             f"loss_type='{loss_type}')")
        self._static_plans = {}
        # Small steps are bound by the HOST (a B = 1 step: ~13 kernel boundaries of one wave of workgroups each behind two eager
        # C-ABI calls): when the same small shape comes `AUTO_STATIC_AFTER` times in a row, calc switches to the captured
        # plan of that shape by itself (ops.StaticFocusCalcFn, automatic mode: images copied out, the eager path again while an
        # earlier calc of the shape still waits for its backward, and for any new shape -- a loader whose batches differ in
        # length never leaves the eager path).  The caller (src/modules/trajectory_net.py:152-158) writes no capture code.
        self.auto_static_shapes = bool(auto_static_shapes)
        self._auto_key, self._auto_run = None, 0
        self._auto_never = set()              # shapes whose plan could not be captured: eager from then on
        self._tmid_dev = {}                   # bin mid-times per device (calc_per_event_basis)
        self._pec_mid_basis = {}              # (device, curve_type, d) -> curve_event_basis at the bin mid-times (calc_per_event_curves)
        # num_tref > 1 (not in the shipped yaml files): the T reference times of a sample as T samples of the num_tref == 1 path
        # (_calc_trefs_as_samples); False: the general kernels (one launch for all reference times, global-atomic event path)
        self.trefs_as_samples = bool(trefs_as_samples)
        self.is_needing_offsets = True
        self.imager = EventImageConverter(self.image_shape)

        assert not scale_iwe_by_dt or num_tref == 1
        assert not polarity_aware_batching or num_tref == 1
        assert not smooth_type == 'on_flow_to_next' or num_tref == 1
        if focus_loss_norm not in ('l1', 'l2') or dist_norm not in ('l1', 'l2'):
            raise ValueError
        if loss_type not in ('gradient_magnitude', 'variance'):
            raise ValueError
        if num_knn > 1 and interpolation_scheme not in ('mean', 'iwd'):
            raise ValueError
        if smooth_weight != 0 and smooth_type not in ('on_flow_to_tref', 'on_flow_to_next'):
            raise ValueError

        self._cfg = ops.PathConfig(
            image_shape=(int(image_shape[0]), int(image_shape[1])), num_tref=int(num_tref),
            num_bins=int(num_bins), num_knn=int(num_knn), smooth_weight=float(smooth_weight),
            sp=int(lut_superpixel_size), norm_l2=(focus_loss_norm == 'l2'), dist_l1=(dist_norm == 'l1'),
            scale_by_dt=bool(scale_iwe_by_dt), mask_border=bool(mask_image_border),
            polarity_split=bool(polarity_aware_batching),
            scheme_iwd=(interpolation_scheme == 'iwd'), smooth_on_next=(smooth_type == 'on_flow_to_next'),
            variance=(loss_type == 'variance'), atomic_path=bool(kwargs.get('debug_atomic_path', False)),
            pyramid_levels=self.pyramid_levels)
        import dataclasses
        self._cfg_t1 = dataclasses.replace(self._cfg, num_tref=1)
        self._cfg_one_level = dataclasses.replace(self._cfg, pyramid_levels=1)      # what ops.PyramidFocusFn runs its level 0 on

    def _calc_trefs_as_samples(self, trajectories, events, t_ref, offsets):
        """num_tref = T > 1 (focus.py:53-57, 66-113) on the kernels of the shipped num_tref == 1 configurations: sample b with its T
        reference times IS T samples (b, 0) .. (b, T - 1) that share b's events and mid-time trajectories and differ in the
        reference-time trajectory -- the same B * T images, the same B * T * num_bins look-up tables, hence the same objective
        (loss.py: a mean over all images) and smoothness (a mean over all tables); the gradient of the shared rows is summed
        by autograd through `repeat_interleave`.  The neighbour search runs T times over the same mid-time points -- twice the
        work of an ideal T-flow kernel for T = 2, a third of the time of the general kernels (C3 shape: 3.73 -> ~1.3 ms).
        Requires what focus.py:49-50 requires of num_tref > 1 anyway (no scale_iwe_by_dt, no polarity_aware_batching)."""
        T = self.num_tref
        b = events.shape[0]
        n = trajectories.shape[2]
        ref = trajectories[:, :T].reshape(b * T, 1, n, 2)
        mid = trajectories[:, T:].repeat_interleave(T, dim=0)
        traj_v = torch.cat((ref, mid), dim=1)
        events_v = events.repeat_interleave(T, dim=0)
        offs_v = offsets.repeat_interleave(T, dim=0) if torch.is_tensor(offsets) else offsets
        return ops.FocusCalcFn.apply(traj_v, events_v, t_ref[:1], self._cfg_t1, -1, offs_v)

    def get_reconstruction_times(self, device):
        """Reference focus.py:53-64: [t_ref..., bin mid-times]."""
        if self.num_tref > 1:
            t_ref = torch.linspace(0, 1, self.num_tref, device=device)
        elif self.num_tref == 1:
            t_ref = torch.rand(1, device=device)  # random reference time
        else:
            raise ValueError("Invalid value for num_tref. Must be >= 1.")

        t_bins = torch.linspace(0, 1, self.num_bins + 1, device=device)
        t_mid = (t_bins[:-1] + t_bins[1:]) / 2
        return torch.concat((t_ref, t_mid), dim=0)

    def _num_pos_events(self, batch, check=True):
        """batch['num_pos_events'], -1 where the batch has none (polarity_aware_batching needs it)."""
        num_pos_events = batch['num_pos_events'] if 'num_pos_events' in batch else -1
        assert not check or not self.polarity_aware_batching or num_pos_events > -1
        return num_pos_events

    @staticmethod
    def _t_ref_on(t_ref, dev):
        """t_ref (scalar tensor / float) as a float32 tensor [1] on `dev`.  No host -> device copy inside the step: a copy from
        pageable memory waits for the stream, and the host then no longer runs ahead of the device -- round 6: 0.86 ms per step of
        which 0.36 were kernels.  A float t_ref becomes a fill kernel."""
        if torch.is_tensor(t_ref):
            return t_ref.to(device=dev, dtype=torch.float32).reshape(1)
        return torch.full((1,), float(t_ref), dtype=torch.float32, device=dev)

    def _bin_mid_times_on(self, dev):
        """The num_bins bin mid-times, kept on every device that asked (no copy inside the step)."""
        tm = self._tmid_dev.get(dev)
        if tm is None:
            from ..utils.synth import bin_mid_times
            tm = self._tmid_dev[dev] = bin_mid_times(self.num_bins).to(dev)
        return tm

    def _own_cell_focus(self, c_rows, phi, events, t_ref, num_pos_events):
        """The per-event warp in plain torch around the vote / objective kernels (cross-check of the fused kernels, and the route
        of a phi that is in the graph): every event moves by the rows [B*G, 2k] of its own LUT cell times phi [B, M, k]
        -> (focus, iwes)."""
        sp, (hq, wq) = self.lut_superpixel_size, self._cfg.lut_grid
        B, M = events.shape[0], events.shape[1]
        with torch.no_grad():
            iy = torch.div(events[..., 0], sp, rounding_mode='floor').long().clamp_(0, hq - 1)      # focus.py:186-187
            ix = torch.div(events[..., 1], sp, rounding_mode='floor').long().clamp_(0, wq - 1)
            idx = (torch.arange(B, device=events.device).view(-1, 1) * (hq * wq) + iy * wq + ix).reshape(-1)
        ce = ops.GatherRowsFn.apply(c_rows, idx).view(B, M, 2, phi.shape[-1])
        warped = events[..., :2] + (ce * phi[:, :, None, :]).sum(-1)                              # [B, M, 2]  (y, x)
        return ops.PrewarpedFocusFn.apply(warped, events, t_ref, self._cfg, int(num_pos_events))

    def _rows_smoothness(self, c_rows, phim, B, in_graph):
        """The smoothness term of the field rows x phim (phim [nbm, k]; None: no term).  in_graph: phim carries a gradient (a table
        that trains) -- BasisFieldFn treats phim as a constant, so the same product in plain torch."""
        if phim is None:
            return torch.zeros((), device=c_rows.device)
        hq, wq = self._cfg.lut_grid
        if in_graph:
            nbm, k = phim.shape
            field = (c_rows.reshape(B * hq * wq * 2, k) @ phim.t()).view(B, hq * wq, 2, nbm).permute(0, 3, 1, 2).reshape(B * nbm, hq, wq, 2)
        else:
            field = ops.BasisFieldFn.apply(c_rows, phim, B, hq, wq)                                # [B*nbm, hq, wq, 2]
        return ops.LutSmoothFn.apply(field, self._cfg, float(self.smooth_weight))

    def _triple(self, loss, focus, smooth, iwes, B):
        """What `calc` returns: (loss with grad, {'focus_loss', 'smoothness_loss'} detached, {'iwes': [B, T, 2, H, W] or
        [B, T, H, W]} detached)."""
        h, w = self._cfg.image_shape
        iwes = iwes.reshape(B, self.num_tref, 2, h, w) if self.polarity_aware_batching else iwes.reshape(B, self.num_tref, h, w)
        return loss, {'focus_loss': focus.detach(), 'smoothness_loss': smooth.detach()}, {'iwes': iwes.detach()}

    def order_events(self, batch):
        """Not in the reference (layout half): `batch` with its event rows ordered by (time bin, LUT
        strip) inside each polarity block and the table `event_offsets` added.  `calc` returns the same loss and
        gradient for the ordered batch bit for bit, and with the table skips one record per event in each direction.
        Meant for the data pipeline: once per batch, next to `utils.ingest_events`."""
        ev, offs = ops.event_bucket_order(self._cfg, batch['events'], int(self._num_pos_events(batch, check=False)))
        out = dict(batch)
        out['events'], out['event_offsets'] = ev, offs
        return out

    def calc_per_event_basis(self, coeff_grid, t_ref, batch, num_basis, basis_type='polynomial', basis_network=None, tile_size=None,
                             fused=True, basis_table=None):
        """UNPINNED EXTENSION -- no reference code exists for it (the reference warps through a binned, KNN-inverted flow LUT,
        focus.py:115-195); BASELINE.json's north_star names it: the per-event continuous-time warp.

        Every event is warped with the motion basis evaluated at ITS OWN timestamp and the coefficients of the tile it lies in:
            warped = (y, x) + sum_k c_k[tile(y, x)] * (basis_k(t_ref) - basis_k(t_event))
        i.e. trajectory_at(t_ref) - trajectory_at(t_event) of the trajectory that STARTS at the event's tile (utils/trajectories.py,
        utils/basis.py) -- no time bins, no nearest-neighbour look-up table; then the reference's weights, bilinear vote, blur and
        objective (focus.py:197-230, event_image_converter.py:333-391, loss.py:4-27) on the HIP kernels.  The smoothness term is
        the reference's Charbonnier term on the same flow sampled at the num_bins bin mid-times.

        coeff_grid [B, 1, 2k, H, W] (first k channels y, next k x: the network's dense output, trajectory_net.py:142-161),
        t_ref scalar tensor / float in [0, 1], batch as for `calc`.  Returns the triple of `calc`.  Differentiable w.r.t. coeff_grid
        (not w.r.t. the weights of a 'learned' basis: the basis values enter as constants -- to TRAIN a basis through this warp, hand
        it over as a table: basis_type='table', below).  With a bucket-ordered batch
        (`order_events` / `ingest_events(order_for=...)`: `event_offsets`) the backward accumulates per LUT strip in LDS fixed point
        and is bitwise reproducible; without the table it uses global float atomics (slow: ~20 G atomics/s, and not
        reproducible).  fused=False: the same in plain torch around the vote / objective kernels (cross-check).

        basis_type='table', basis_table=T: the basis is T [S + 1, num_basis] (fp32, on the events' device), samples at the knots
        i / S interpolated linearly at every event's time (utils.table_basis_values is the definition; utils.basis_table samples any
        basis of utils.basis_values, e.g. T = basis_table('learned', k, 1024, net)).  Differentiable w.r.t. coeff_grid AND T: the
        kernels read the table and reduce the whole batch's gradient onto its (S + 1) * num_basis entries (bitwise reproducible in
        either event layout); ordinary autograd carries it on into the weights of `net`, or T is an nn.Parameter itself.  The fused
        node serves what the library says it serves (num_basis <= 8, num_bins <= 64, a table within its LDS limit); anything else,
        and fused=False, runs in plain torch around the vote / objective kernels with the same gradients from autograd.

        A tile without a centre: there are ceil(H / sp) x ceil(W / sp) cells, and where 0 < H % sp <= sp // 2 (W likewise) the
        centre sp // 2 of the last row (column) of cells lies outside the image.  Such a cell carries zero coefficients: its
        events are not warped, it enters the smoothness field with zero flow, and no element of coeff_grid receives its
        gradient.

        An fp16 / bf16 coeff_grid (a network under autocast, a .half() / .bfloat16() model) is read by the fused node as it is -- no
        .float() copy; the conversion at the load is exact, so loss and images are those of coeff_grid.float(), bit for bit -- and
        its gradient comes back in the grid's dtype, computed in fp32 and rounded once (round to nearest even)."""
        from ..utils import basis_values, table_basis_values
        if self.num_tref != 1:
            raise ValueError('calc_per_event_basis needs num_tref == 1')
        events = batch['events']
        if (basis_type == 'table') != (basis_table is not None):
            raise ValueError("basis_type='table' and basis_table go together")
        if basis_table is not None:
            if not (torch.is_tensor(basis_table) and basis_table.dim() == 2 and basis_table.dtype == torch.float32
                    and basis_table.device == events.device and basis_table.shape[0] >= 2):
                raise ValueError("basis_table must be a 2-D float32 tensor [samples + 1, num_basis] on the events' device")
            if basis_table.shape[1] != num_basis:
                raise ValueError(f'basis_table has {basis_table.shape[1]} columns, num_basis is {num_basis}')
        num_pos_events = self._num_pos_events(batch)
        dev = events.device
        sp = self.lut_superpixel_size
        tile = sp if tile_size is None else int(tile_size)
        if tile != sp:
            raise ValueError('the coefficient tiles must be the look-up-table cells (tile_size == lut_superpixel_size)')
        hq, wq = self._cfg.lut_grid
        B = events.shape[0]
        # the coefficients at the tile centres (get_optical_flow_tile_mask + coeffs_grid_to_list, trajectories.py:3-52: offset
        # tile // 2, row-major -- as a strided view, whose backward is a strided copy), scales summed as compute_basis does
        if coeff_grid.dim() != 5 or coeff_grid.shape[2] != 2 * num_basis or -(-coeff_grid.shape[3] // tile) != hq or -(-coeff_grid.shape[4] // tile) != wq:
            raise ValueError(f'coeff_grid {tuple(coeff_grid.shape)} is not [B, scales, {2 * num_basis}, H, W] of this image shape')
        t_ref = self._t_ref_on(t_ref, dev)
        offsets = batch['event_offsets'] if 'event_offsets' in batch else None     # from order_events / ingest (optional)
        # a table: the fused node where the library serves (k, num_bins, table size) -- the kernels read the table --, else the
        # plain-torch chain below with phi from the table INSIDE the graph (autograd carries its gradient to the table)
        tab_fused = basis_table is not None and bool(fused) and ops.pe_table_supported(self._cfg, events, int(num_pos_events), num_basis,
                                                                                      basis_table.shape[0] - 1)
        if basis_table is not None and not tab_fused:
            fused = False
        phi = None           # (fused + polynomial basis of up to 8 orders, or a table: worked out inside the kernels)
        if basis_table is not None:
            if not tab_fused:
                phi = table_basis_values(basis_table, t_ref) - table_basis_values(basis_table, events[..., 2])
        elif not (fused and basis_type == 'polynomial' and num_basis <= 8):
            with torch.no_grad():
                phi = basis_values(t_ref, num_basis, basis_type, basis_network) - basis_values(events[..., 2], num_basis, basis_type, basis_network)
        phim = None
        if self.smooth_weight > 0:
            tm = self._bin_mid_times_on(dev)
            if basis_table is not None:
                bv = table_basis_values(basis_table, torch.cat((t_ref, tm)))       # (one evaluation for t_ref and the mid-times: half the operators)
                phim = bv[:1] - bv[1:]                                               # [nb, k], in the graph
            else:
                with torch.no_grad():
                    phim = basis_values(t_ref, num_basis, basis_type, basis_network) - basis_values(tm, num_basis, basis_type, basis_network)   # [nb, k]
        if tab_fused:
            loss, focus, smooth, iwes = ops.PerEventBasisCalcFn.apply(coeff_grid, events, None, phim, t_ref, self._cfg, int(num_pos_events), offsets,
                                                                      int(num_basis), tile, basis_table)
            return self._triple(loss, focus, smooth, iwes, B)
        if fused and num_basis <= 8 and self.num_bins <= 64:
            # one autograd node of library calls (ops.PerEventBasisCalcFn): the step is no longer bound by the host
            loss, focus, smooth, iwes = ops.PerEventBasisCalcFn.apply(coeff_grid, events, phi, phim, t_ref, self._cfg, int(num_pos_events), offsets,
                                                                      int(num_basis), tile)
            return self._triple(loss, focus, smooth, iwes, B)
        c_rows = ops.TileCoeffRowsFn.apply(coeff_grid, tile)                                       # [B*G, 2k]: per tile (y: k, x: k)
        if fused:
            focus, iwes = ops.PerEventBasisFocusFn.apply(c_rows, events, phi, t_ref, self._cfg, int(num_pos_events), offsets)
        else:
            focus, iwes = self._own_cell_focus(c_rows, phi, events, t_ref, num_pos_events)
        smooth = self._rows_smoothness(c_rows, phim, B, in_graph=basis_table is not None)
        return self._triple(focus + smooth, focus, smooth, iwes, B)

    PEC_TILES = (2, 4, 8, 16)

    def _curve_tile_grid(self, params, up_mask, scale):
        """The checks of calc_per_event_curves that need no device: -> (d, tile).  Every rule raises a ValueError that names it."""
        if self.num_tref != 1:
            raise ValueError('calc_per_event_curves needs num_tref == 1')
        if not torch.is_tensor(params) or params.dim() != 4 or params.shape[1] % 2 or params.shape[1] < 2:
            raise ValueError(f'params must be [B, 2d, h, w] (control points 1..d, x channels first), got {tuple(getattr(params, "shape", ()))}')
        B, c2, h, w = params.shape
        sp, scale = self.lut_superpixel_size, float(scale)
        if not scale > 0:
            raise ValueError(f'scale must be positive, got {scale}')
        tile = int(round(sp / scale))
        if tile not in self.PEC_TILES or abs(tile * scale - sp) > 1e-6 * sp:
            raise ValueError(f'tile = lut_superpixel_size / scale = {sp} / {scale} must be one of {self.PEC_TILES}')
        hq, wq = self._cfg.lut_grid
        if up_mask is not None:
            if not torch.is_tensor(up_mask) or tuple(up_mask.shape) != (B, 576, h, w):
                raise ValueError(f'up_mask must be [B, 576, h, w] = {(B, 576, h, w)}, got {tuple(getattr(up_mask, "shape", ()))}')
            if (8 * h) % tile or (8 * w) % tile or (8 * h // tile, 8 * w // tile) != (hq, wq):
                raise ValueError(f'the tile grid of the 8h x 8w = {8 * h} x {8 * w} image at tile {tile} must equal the look-up-table grid {hq} x {wq}')
        elif (h, w) != (hq, wq):
            raise ValueError(f'without up_mask the grid of params is the tile grid and must equal the look-up-table grid {hq} x {wq}, got {h} x {w}')
        return c2 // 2, tile

    def calc_per_event_curves(self, params, t_ref, batch, *, up_mask=None, curve_type='BEZIER', basis_table=None, scale=1.0, fused=True,
                              basis_network=None, table_samples=1024):
        """UNPINNED EXTENSION (BASELINE.json's north_star and configs[3]): the per-event continuous-time warp along RAFT-spline
        curves.  Every event moves along the curve of the tile it lies in, evaluated at ITS OWN timestamp -- no time bins, no KNN
        look-up table, time not piecewise constant (`trajectories_from_bezier(up_mask=)` + `calc` is that route).

        params [B, 2d, h, w]: control points 1..d, x in the first d channels, y in the next d (reference curves/polynomial.py:60-61;
        P0 = 0).  With up_mask [B, 576, h, w] they live on the 1/8 grid and are upsampled as reference raft_spline/utils.py:30-45
        does; without it they are per tile already (h x w = the tile grid).  t_ref scalar tensor / float, batch as for `calc`.
          rows[(b, cell)][0][j] = scale * up_y[j],  rows[(b, cell)][1][j] = scale * up_x[j]   at the tile centres
              (iy * tile + tile // 2, ix * tile + tile // 2) of the 8h x 8w image; tile = lut_superpixel_size / scale, one of 2, 4, 8,
              16; the tile grid must equal the look-up-table grid (EVIMO2: 384 x 512 net, 480 x 640 events, scale 1.25, sp 5, tile 4)
          warped = (y, x) + sum_j rows[cell(y, x)][:, j] * phi_j,   phi_j = E_j(t_ref) - E_j(t_event)      (j ascending)
        with E of `utils.curve_event_basis`: curve_type 'BEZIER' (1 <= d), 'POLYNOMIAL', 'BSPLINE' (the clamped cubic B-spline of
        d + 1 control points, evaluated exactly: 3 <= d, ValueError below; at most 8 of the d coefficient pairs are read per event),
        or 'TABLE' with basis_table [S + 1, d] (a frozen learned basis, say -- or one that trains: below).  Then the reference's weights,
        vote, blur and objective; the smoothness term is the reference's Charbonnier term on rows x phim with
        phim[t] = E(t_ref) - E(t_mid[t]) ('on_flow_to_tref') or E(t_mid[t + 1]) - E(t_mid[t]) ('on_flow_to_next').
        Returns the triple of `calc`.  Gradients go to params and up_mask -- and to basis_table where it requires grad (and grad
        mode is on): d loss / d T through the events, where with (gy, gx) the position gradient of a row, G_j = gy * rows[cell][0][j]
        + gx * rows[cell][1][j], (i, f) the interval of the row's time and (ir, fr) that of t_ref, T's gradient gets -(1 - f) G_j at
        [i][j], -f G_j at [i + 1][j], +(1 - fr) G_j at [ir][j] and +fr G_j at [ir + 1][j] (rows of weight 0 add nothing), and through
        the smoothness term, whose phim is then built inside the graph with `utils.table_basis_values`.  A table that does not
        require grad is a constant and runs exactly what it ran before.
        curve_type='LEARNED', basis_network=net, table_samples=S (default 1024): the reference's learned curve (curves/learned.py:
        76-77) tabulated -- shorthand for curve_type='TABLE', basis_table=utils.curve_basis('LEARNED', arange(S + 1) / S, d, net): the
        network runs at the S + 1 knots inside the graph, and autograd carries the table's gradient into its parameters.
        The fused node serves (S + 1) * d <= mpc_pe_table_limit() = 16384: at d = 16 the default table_samples = 1024 is ONE knot
        past it (16400) and takes the plain-torch route, roughly 10 to 40 times slower -- pass table_samples <= 1023 there (d = 10: up to
        1637).  The table is moved to the events' device; a caller's own basis_table on another device is not, and leaves the node.

        fused=True: one autograd node (ops.PerEventCurvesFn, csrc/pe_curves.hip), the basis evaluated in registers; with a
        bucket-ordered batch (`event_offsets`) the backward sums per LUT strip in LDS fixed point, bitwise reproducible, in
        ceil(d / orders per pass) passes; without the table it uses global float atomics (slow, not reproducible).
        fused=False, and whatever the library refuses (d > 16, a table past mpc_pe_table_limit(), num_bins > 64, a CPU basis_table):
        phi [B, M, d] and the rows in plain torch around the existing per-event nodes (the cross-check).  A table that trains is
        served by the fused node wherever a constant one is (mpc_pec_table_basis_grad: one more streaming pass, Q33.30 sums, bitwise
        reproducible in either event layout; |G_j| < 2^31 and a knot's sum over the batch below 2^33); elsewhere phi stays in the
        graph and plain torch around the vote / objective kernels delivers the same three gradients.  No graph capture.
        An fp16 / bf16 up_mask (a network under autocast) is read by the fused node as it is -- no .float() copy, the same loss bits
        as for the upcast mask -- and gets its gradient in its own dtype, computed in fp32 and rounded once; params that are not
        fp32 go through a differentiable .float()."""
        from ..utils import curve_event_basis, curve_head_rows, curve_basis, table_basis_values
        from ..utils.basis import CURVE_EVENT_TYPES, BSPLINE_MIN_DEGREE
        d, tile = self._curve_tile_grid(params, up_mask, scale)
        if curve_type == 'LEARNED':
            if basis_table is not None:
                raise ValueError("curve_type='LEARNED' builds its own table from basis_network: pass no basis_table")
            if basis_network is None:
                raise ValueError("curve_type='LEARNED' needs basis_network")
            S = int(table_samples)
            if S < 1:
                raise ValueError(f'table_samples must be >= 1, got {table_samples}')
            net_dev = next((p.device for p in basis_network.parameters()), batch['events'].device)
            # (the network at the knots i / S, inside the graph; a wrong output width raises in curve_basis)
            basis_table = curve_basis('LEARNED', torch.arange(S + 1, dtype=torch.float32, device=net_dev) / float(S), d, basis_network)
            # (a network on another device than the events: the table moves, inside the graph, and the fused node still serves it)
            basis_table = basis_table.to(batch['events'].device)
            curve_type = 'TABLE'
        if curve_type not in CURVE_EVENT_TYPES:
            raise ValueError(f'curve_type must be one of {CURVE_EVENT_TYPES}, got {curve_type!r}')
        if (curve_type == 'TABLE') != (basis_table is not None):
            raise ValueError("curve_type='TABLE' and basis_table go together")
        if curve_type == 'BSPLINE' and d < BSPLINE_MIN_DEGREE:
            raise ValueError(f"curve_type='BSPLINE' is cubic: it needs d >= {BSPLINE_MIN_DEGREE} control points per axis beside P0, got {d}")
        if basis_table is not None and not (torch.is_tensor(basis_table) and basis_table.dim() == 2 and basis_table.dtype == torch.float32
                                            and basis_table.shape[0] >= 2 and basis_table.shape[1] == d):
            raise ValueError(f'basis_table must be a 2-D float32 tensor [samples + 1, d = {d}]')
        events = batch['events']
        if events.shape[0] != params.shape[0]:
            raise ValueError(f'params hold {params.shape[0]} samples, the events {events.shape[0]}')
        num_pos_events = self._num_pos_events(batch)
        dev = events.device
        B = events.shape[0]
        t_ref = self._t_ref_on(t_ref, dev)
        offsets = batch['event_offsets'] if 'event_offsets' in batch else None
        if fused and basis_table is not None and basis_table.device != dev:
            fused = False
        if fused and not ops.pec_supported(self._cfg, events, int(num_pos_events), d, curve_type,
                                           basis_table.shape[0] - 1 if basis_table is not None else 0) & 1:
            fused = False
        # a table that TRAINS stays in the graph; any other is the constant it was
        trains = basis_table is not None and basis_table.requires_grad and torch.is_grad_enabled()
        if basis_table is not None:
            basis_table = basis_table.to(dev) if trains else basis_table.detach().to(dev)
        phim = None
        if self.smooth_weight > 0:
            tm = self._bin_mid_times_on(dev)
            if trains:
                # (in the graph: the lines of curve_event_basis('TABLE'), the same bits)
                if self.smooth_type == 'on_flow_to_next':
                    em = table_basis_values(basis_table, tm)
                    phim = em[1:] - em[:-1]
                else:
                    bv = table_basis_values(basis_table, torch.cat((t_ref, tm)))    # (one evaluation for t_ref and the mid-times)
                    phim = bv[:1] - bv[1:]
            else:
                with torch.no_grad():
                    # (the basis at the bin mid-times is a constant of (curve, d): kept -- the torch lines of the B-spline are ~80 small
                    # launches, 0.3 ms of host time per step; a table is the caller's and may change between calls)
                    key = (dev, curve_type, d)
                    em = self._pec_mid_basis.get(key) if basis_table is None else None
                    if em is None:
                        em = curve_event_basis(tm, d, curve_type, basis_table)
                        if basis_table is None:
                            if len(self._pec_mid_basis) >= 16:
                                self._pec_mid_basis.clear()
                            self._pec_mid_basis[key] = em
                    phim = (em[1:] - em[:-1]) if self.smooth_type == 'on_flow_to_next' else (curve_event_basis(t_ref, d, curve_type, basis_table) - em)
            if phim.shape[0] == 0:
                phim = None
        if fused:
            if params.dtype != torch.float32:
                params = params.float()           # (differentiable: autograd casts grad_params back; the mask is read in its own dtype)
            loss, focus, smooth, iwes = ops.PerEventCurvesFn.apply(params, up_mask, events, t_ref, phim, self._cfg, int(num_pos_events), offsets,
                                                                   curve_type, basis_table, float(scale), tile)
        elif trains:
            # plain torch around the vote / objective kernels with phi INSIDE the graph (autograd carries its gradient to the table):
            # the chain of calc_per_event_basis for a table the library does not serve, and the cross-check of the fused node
            phi = table_basis_values(basis_table, t_ref) - table_basis_values(basis_table, events[..., 2])
            c_rows = curve_head_rows(params, up_mask, scale, tile)
            focus, iwes = self._own_cell_focus(c_rows, phi, events, t_ref, num_pos_events)
            smooth = self._rows_smoothness(c_rows, phim, B, in_graph=True)
            loss = focus + smooth
        else:
            with torch.no_grad():
                phi = curve_event_basis(t_ref, d, curve_type, basis_table) - curve_event_basis(events[..., 2], d, curve_type, basis_table)
            c_rows = curve_head_rows(params, up_mask, scale, tile)
            focus, iwes = ops.PerEventBasisFocusFn.apply(c_rows, events, phi, t_ref, self._cfg, int(num_pos_events), offsets)
            smooth = self._rows_smoothness(c_rows, phim, B, in_graph=False)
            loss = focus + smooth
        return self._triple(loss, focus, smooth, iwes, B)

    AUTO_STATIC_MAX_EVENTS = 150_000     # B * M up to which the captured plan wins (C2: 0.16 against 0.20 ms; C4, 500k events: it loses)
    AUTO_STATIC_AFTER = 3                 # consecutive calcs of one shape before it is captured

    def _auto_static(self, trajectories, events, num_pos_events, offsets):
        """Should this calc replay the captured plan of its shape?  (automatic static shapes, see __init__)"""
        if not self.auto_static_shapes or self.profiler is not None or ops.STAGE_TIMER is not None or ops.kernel_timer_on():
            return False
        if not (torch.is_tensor(events) and events.is_cuda and events.dim() == 3 and torch.is_tensor(trajectories) and trajectories.is_cuda
                and trajectories.dim() == 4):
            return False                  # (the eager path raises the proper error)
        if ops.knn_is_wide(trajectories.shape[2]):
            return False                  # (n >= 65536: the chunked neighbour search has no captured form)
        if events.shape[0] * events.shape[1] > self.AUTO_STATIC_MAX_EVENTS or torch.cuda.is_current_stream_capturing():
            return False
        key = ops.StaticFocusCalcFn.plan_key(trajectories, events, self._cfg, int(num_pos_events), offsets)
        if key in self._auto_never:
            return False
        if key == self._auto_key:
            self._auto_run += 1
        else:
            self._auto_key, self._auto_run = key, 1
        if self._auto_run < self.AUTO_STATIC_AFTER:
            return False
        return not ops.StaticFocusCalcFn.plan_busy(self._static_plans, key)

    def calc(self, trajectories, times, batch):
        """Reference focus.py:66-113.

        trajectories [B, num_tref + num_bins, n, 2] (y, x), times [num_tref + num_bins],
        batch['events'] [B, M, 6], batch['num_pos_events'] (int, with polarity_aware_batching).
        Returns (loss with grad, {'focus_loss', 'smoothness_loss'} detached,
                 {'iwes': [B, T, 2, H, W] or [B, T, H, W]} detached)."""
        events = batch['events']
        num_pos_events = self._num_pos_events(batch)

        t_ref = times[:self.num_tref]
        offsets = batch['event_offsets'] if 'event_offsets' in batch else None     # from order_events (optional)
        if self.num_tref > 1 and self.trefs_as_samples and not self._cfg.atomic_path and torch.is_tensor(events) and events.dim() == 3 \
                and torch.is_tensor(trajectories) and trajectories.dim() == 4:
            out = self._calc_trefs_as_samples(trajectories, events, t_ref, offsets)
        elif self.pyramid_levels > 1 and not self.pyramid_fused:
            out = ops.PyramidFocusFn.apply(trajectories, events, t_ref, self._cfg_one_level, int(num_pos_events), self.pyramid_levels)
        elif self.static_shapes and ops.STAGE_TIMER is None and not torch.cuda.is_current_stream_capturing():
            out = ops.StaticFocusCalcFn.apply(trajectories, events, t_ref, self._cfg, int(num_pos_events), offsets, self._static_plans)
        elif self._auto_static(trajectories, events, num_pos_events, offsets):
            try:
                out = ops.StaticFocusCalcFn.apply(trajectories, events, t_ref, self._cfg, int(num_pos_events), offsets, self._static_plans, True)
            except ops.AutoPlanFailed:
                # the plan of this shape could not be captured (another thread of the training process used the device in the
                # capture window, no memory for the plan's buffers, ...): this step and every later one of the shape run eagerly
                self._auto_never.add(ops.StaticFocusCalcFn.plan_key(trajectories, events, self._cfg, int(num_pos_events), offsets))
                out = ops.FocusCalcFn.apply(trajectories, events, t_ref, self._cfg, int(num_pos_events), offsets)
        elif self.profiler is not None:
            with torch.profiler.record_function('mpcmax::FocusLoss.calc'):
                out = ops.FocusCalcFn.apply(trajectories, events, t_ref, self._cfg, int(num_pos_events), offsets)
        else:
            out = ops.FocusCalcFn.apply(trajectories, events, t_ref, self._cfg, int(num_pos_events), offsets)
        return self._triple(*out, events.shape[0])
