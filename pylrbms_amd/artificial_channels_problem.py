"""Artificial channels problem (reference python/dune/pylrbms/artificial_channels_problem.py), the data of the reference's
parabolic demo python/scripts/parabolic.py.

Omega = [0, 1]^2 with four channels of width 1/16 along y = 1/8, 3/8, 5/8, 7/8 (x in [1/16, 15/16]), joined at both ends by
vertical connections: fixed ones between the channels 1-2 and 3-4, switched ones (coefficient ``switch``) between 2-3.
Diffusion lambda(mu) = mu_min background + mu_max (channels + fixed connections) + switch (switched connections), kappa = I.
Source f(t) = phi_0(t) f_top_left + phi_1 f_right with phi_0(t) = [sin(4 pi t) > 0] (the top-left connection feeds while it
is on) and phi_1 = -1 (the two right connections drain).  Every data function is an indicator function (value decided by
the element centre, closed boxes: DESIGN.md section 3).

``half_num_fine_elements_per_subdomain_and_dim`` must be > 3 (``make_grid`` asserts it, as the reference's grid.py does), so
the demo's own configuration (``half = 2``) is refused here as it is there; the channels are resolved from ``half = 8``
on (element centres at spacing 1/48 across a channel of width 1/16).
"""
from pylrbms_amd.functions import make_constant_function_1x1, make_constant_function_2x2, make_indicator_function_1x1
from pylrbms_amd.grid import make_boundary_info, make_grid
from pylrbms_amd.parameters import ExpressionParameterFunctional, ProjectionParameterFunctional

W = 1.0 / 32.0      # half channel width
E = 1.0 / 16.0      # distance of the channel ends from the boundary


def horizontal_channels(value):
    return [[[[E, y - W], [1 - E, y + W]], value] for y in (1 / 8, 3 / 8, 5 / 8, 7 / 8)]


def fixed_vertical_connections(value):
    """Between channels 1-2 and 3-4, at both ends."""
    return [[[[x0, y0 + W], [x1, y1 - W]], value]
            for (x0, x1) in ((E, 1 / 4 - E), (3 / 4 + E, 1 - E))
            for (y0, y1) in ((1 / 8, 3 / 8), (5 / 8, 7 / 8))]


def switched_vertical_connections(value):
    """Between channels 2-3, at both ends."""
    return [[[[x0, 3 / 8 + W], [x1, 5 / 8 - W]], value] for (x0, x1) in ((E, 1 / 4 - E), (3 / 4 + E, 1 - E))]


def init_grid_and_problem(config, mu_bar=(1,), mu_hat=(1,), mpi_comm=None, switch_off_after=None):
    """``switch_off_after=t*``: the switched connections carry ``switch`` for ``_t <= t*`` and ``mu_min`` afterwards -- they close
    during the run (a diffusion coefficient of the time, parabolic path only).  None: open throughout."""
    lower_left, upper_right = [0, 0], [1, 1]
    mu_bar, mu_hat = tuple(mu_bar), tuple(mu_hat)
    mu_min = min((0.01,) + mu_bar + mu_hat)
    mu_max = max((1,) + mu_bar + mu_hat)
    inner_boundary_id = 18446744073709551573
    grid = make_grid((lower_left, upper_right), config['num_subdomains'],
                     config['half_num_fine_elements_per_subdomain_and_dim'], inner_boundary_id, mpi_comm=mpi_comm)
    all_dirichlet_boundary_info = make_boundary_info(grid, {'type': 'xt.grid.boundaryinfo.alldirichlet'})

    channels = make_indicator_function_1x1(grid, horizontal_channels(1), 'horizontal_channels')
    fixed = make_indicator_function_1x1(grid, fixed_vertical_connections(1), 'fixed_vertical_connections')
    switched = make_indicator_function_1x1(grid, switched_vertical_connections(1), 'switched_vertical_connections')
    background = make_constant_function_1x1(grid, 1) - channels - fixed - switched

    parameter_type = {'switch': (1,)}
    lambda_functions = [background, channels, fixed, switched]
    lambda_coefficients = [ExpressionParameterFunctional(str(mu_min), parameter_type),
                           ExpressionParameterFunctional(str(mu_max), parameter_type),
                           ExpressionParameterFunctional(str(mu_max), parameter_type),
                           ProjectionParameterFunctional(component_name='switch', component_shape=(1,), coordinates=(0,))]
    if switch_off_after is not None:
        lambda_coefficients[3] = ExpressionParameterFunctional(
            'switch if _t <= {!r} else {!r}'.format(float(switch_off_after), float(mu_min)), {'switch': (1,), '_t': ()})
    kappa = make_constant_function_2x2(grid, [[1., 0.], [0., 1.]], name='kappa')
    top_left = [b for b in fixed_vertical_connections(1) if b[0][0][0] < 0.5 and b[0][0][1] > 0.5]
    right = [b for b in fixed_vertical_connections(1) if b[0][0][0] > 0.5]
    f_functions = [make_indicator_function_1x1(grid, top_left, 'top_left'),
                   make_indicator_function_1x1(grid, right, 'right')]
    f_coefficients = [ExpressionParameterFunctional('sin(2 * 2 * pi * _t) > 0', {'_t': ()}),
                      ExpressionParameterFunctional('-1', None)]

    def create_lambda(mu):
        """lambda(mu) as one function: the constant mu_min with every channel / connection box replaced by its value."""
        return (make_constant_function_1x1(grid, mu_min)
                - make_indicator_function_1x1(grid, horizontal_channels(mu_min))
                - make_indicator_function_1x1(grid, fixed_vertical_connections(mu_min))
                - make_indicator_function_1x1(grid, switched_vertical_connections(mu_min))
                + make_indicator_function_1x1(grid, horizontal_channels(mu_max))
                + make_indicator_function_1x1(grid, fixed_vertical_connections(mu_max))
                + make_indicator_function_1x1(grid, switched_vertical_connections(mu[0])))

    return {'grid': grid,
            'mpi_comm': mpi_comm,
            'boundary_info': all_dirichlet_boundary_info,
            'inner_boundary_id': inner_boundary_id,
            'lambda': {'functions': lambda_functions, 'coefficients': lambda_coefficients},
            'lambda_bar': create_lambda(mu_bar),
            'lambda_hat': create_lambda(mu_hat),
            'kappa': kappa,
            'f': {'functions': f_functions, 'coefficients': f_coefficients},
            'parameter_type': parameter_type,
            'mu_bar': mu_bar,
            'mu_hat': mu_hat,
            'mu_min': (mu_min,),
            'mu_max': (mu_max,),
            'parameter_range': (mu_min, mu_max)}

