materials {
	{
		shininess	= 0,
		diffuse		= (0, 0, 0),
		specular	= (0, 0, 0),
		ambient		= (0.01, 0.01, 0.02)
	},

	{
		shininess	= 12,
		diffuse		= (0.3, 0.2, 0.15),
		specular	= (0.2, 0.2, 0.2),
		ambient		= (0.1, 0.08, 0.06)
	},

	{
		shininess	= 40,
		diffuse		= (0.1, 0.15, 0.25),
		specular	= (0.3, 0.3, 0.35),
		ambient		= (0.04, 0.05, 0.08)
	}
}

scene {
	ambient {
		color = (0.05, 0.05, 0.05)
	},

	camera {
		point		= (0, 3, 5),
		direction	= (0, -0.4, -1),
		fov		= 100
	},

	point_light {
		point			= (-4, 6, 1),
		diffuse_intensity	= (2, 1.8, 1.5),
		specular_intensity	= (2, 2, 2)
	},

	point_light {
		point			= (5, 4, -2),
		diffuse_intensity	= (0.5, 0.9, 1.6),
		specular_intensity	= (1, 1, 1.5)
	},

	point_light {
		point			= (0, 9, -7),
		diffuse_intensity	= (1.2, 1.2, 1.2),
		specular_intensity	= (0.5, 0.5, 0.5)
	},

	smooth-union {
		smoothness	= 1.5,
		material	= #1,
		a = sphere {
			point		= (-1, 0.5, -3),
			radius		= 1.5
		},
		b = sphere {
			point		= (1.2, 0.2, -4),
			radius		= 1
		}
	},

	sphere {
		point		= (2.5, 1.5, -1.5),
		radius		= 0.7,
		material	= #2
	},

	plane {
		y		= -1,
		material	= #2
	}
}
