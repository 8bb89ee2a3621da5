"""Regression bases for Longstaff-Schwartz (reference: maths/regression.py:3-14)."""
import torch


class RegressionFunction:
    def __init__(self, degree):
        self.degree = degree

    def get_degree(self):
        # number of basis functions, as in the reference (degree + 1)
        return self.degree + 1


class PolyomialRegression(RegressionFunction):  # (sic) the reference's spelling is part of its API
    """Monomial basis [x^0 .. x^degree]."""

    def get_regression_matrix(self, explanatory_variables: torch.Tensor) -> torch.Tensor:
        cols = [torch.ones_like(explanatory_variables)]
        for _ in range(self.degree):
            cols.append(cols[-1] * explanatory_variables)
        return torch.stack(cols, dim=1)


PolynomialRegression = PolyomialRegression


def regression_centering(x_range, x):
    """(shift, scale, degenerate) of the explanatory atom x: z = (x - shift) * scale maps its range over all ranks to [-1, 1];
    degenerate: every path at one value (a regression at the calibration date).  x_range: {x atom: (min, max)}"""
    xmin, xmax = x_range[x]
    degenerate = not (xmax > xmin)
    shift = 0.5 * (xmin + xmax) if not degenerate else xmin
    scale = 2.0 / (xmax - xmin) if not degenerate else 1.0
    return shift, scale, degenerate
